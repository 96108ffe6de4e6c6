"""``matlab/main_channel_mask.m`` as functions -- SURVEY.md 8f row f1.

The BER experiment of main_BER_calculation.m run twice on the same data: as is, and with every
windowed symbol passed through a DFT-domain raised-cosine "channel mask" before the overlap-add;
in both only the centre half of the spectrum carries data.  The frame loop runs on the GPU:
``Plan.set_allocation`` (zero padding + ifftshift of lines 387-390, bin selection of 367-369) and
``Plan.set_tx_mask`` (``dft_rc_filt``, 398-417).  ``spectrum_for_window_file`` is the spectrum side of the same
experiment: the periodogram and out-of-band radiation of the plain and of the masked waveform
(``wofdm_tx_psd_batch_masked``); ``interference_for_window_file`` is its deterministic side, the closed-form ICI +
ISI power of the same two systems (``wofdm_interference_masked``): what the mask costs next to what it buys.
``papr_for_window_file`` is the envelope side: the PAPR histogram and CCDF of the plain and of the masked frames
(``wofdm_tx_papr``).  ``profile_for_window_file`` shows where in the band the errors of the two systems sit: bit errors,
symbol errors and error-vector power per subcarrier (``wofdm_rx_profile``).  ``pa_for_window_file`` puts both systems behind
a nonlinear power amplifier: the profile and the spectral regrowth per back-off (``wofdm_rx_profile_pa``,
``wofdm_tx_psd_batch_pa``).

BER is accumulated over the whole ensemble here as there (lines 341-359).  The reference sends
the same data bits through both runs with independent noise (two ``add_wgn`` calls); here the
plain and the masked run simply use disjoint frame ranges (independent bits and noise), which
leaves every BER estimate unbiased.
"""
import os

import numpy as np

from . import simulation as S
from . import variants as V

ROLL_OFF = 10             # main_channel_mask.m:54


def half_band_allocation(n_fft):
    """Loaded bins of lines 387-390: ``[zeros(offset) data zeros(offset)]`` with offset = N/4
    (line 53), centred spectrum -> after ifftshift the data sit on bins [0, N/4) and [3N/4, N)."""
    a = np.zeros(n_fft, dtype=bool)
    a[:n_fft // 4] = True
    a[3 * n_fft // 4:] = True
    return a


def gen_raised_cosine(window_length, roll_off, total_length):
    """Centred raised-cosine mask (lines 443-458): zeros | rising sin^2 edge of ``roll_off``
    samples | ``window_length`` ones | falling edge | zeros."""
    axis = np.arange(-(roll_off + 1) / 2 + 1, (roll_off + 1) / 2 - 1 + 0.5, 1.0)
    rc = np.sin(np.pi / 2 * (0.5 + axis / roll_off)) ** 2
    rest = total_length - window_length - 2 * roll_off
    return np.concatenate([np.zeros(rest // 2), rc, np.ones(window_length), rc[::-1],
                           np.zeros(rest - rest // 2)])


def tx_mask(sym_len, roll_off=ROLL_OFF):
    """DFT-domain gains of ``dft_rc_filt`` in natural bin order (lines 402-405):
    ``ifftshift(gen_raised_cosine(floor((2P-1)/2), rollOff, 2P-1))``."""
    L = 2 * sym_len - 1
    return np.fft.ifftshift(gen_raised_cosine(L // 2, roll_off, L))


def dft_rc_filt(rows, roll_off=ROLL_OFF):
    """Host restatement of lines 398-417 on [S, P] rows (numpy FFT of length 2P-1): used by the
    tests as an independent check of the mask stage."""
    rows = np.asarray(rows, dtype=np.complex128)
    n_sym, P = rows.shape
    L = 2 * P - 1
    y = np.fft.ifft(np.fft.fft(rows, L, axis=1) * tx_mask(P, roll_off)[None, :], axis=1)
    out = y[:, :P].copy()
    out[1:, :P - 1] += y[:-1, P:]
    return out


def _frames(ensemble, frame_range):
    """(first frame, count): the whole ensemble, or ``frame_range`` as given"""
    return (0, ensemble) if frame_range is None else frame_range


def _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off=ROLL_OFF, rx=True):
    """What every ``*_for_window_file`` function begins with: the structure (a tail only on the side the system windows), the
    pair plan, the windows of every pair of the file + the RC pair, w_tx [pairs, P] and w_rx [pairs, N + delta], the half-band
    allocation and the Tx mask.  rx=False (the Tx-side functions, whose window files need not hold the Rx windows): w_rx is
    None."""
    st = V.make_structure(type_ofdm, num_subcar, cp, tail_tx if type_ofdm in V.TX_WINDOWED else 0,
                          tail_rx if type_ofdm in V.RX_WINDOWED else 0)
    rc = (V.tx_rc_window(st), V.rx_rc_window(st))
    plan = V.matlab_pair_plan(type_ofdm)

    def stack(side):
        return np.stack([rc[side] if k[side] == "rc" else np.asarray(windows[k[side]], dtype=np.float64) for _, k in plan])
    return st, plan, stack(0), stack(1) if rx else None, half_band_allocation(num_subcar), tx_mask(st.sym_len, roll_off)


def _profiles_per_pair(arm, plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(), tail_masked=None, **kw):
    """What the receive-profile functions end with: ``rx_profile.rx_profile<arm>_gpu`` (gpu=False: ``..._host``, which takes
    no device) on the frames of ``_frames``, plain and masked, and the result per pair of the plan -- {name: {"profile",
    "profile_masked"}}, each the route's namedtuple without the pair axis.  head: the arguments before (first, count); tail:
    the arm's own behind them (tail_masked: those of the masked call, where they differ); kw: its keywords."""
    from . import rx_profile as R
    first, count = _frames(ensemble, frame_range)
    run = getattr(R, "rx_profile%s_%s" % (arm, "gpu" if gpu else "host"))
    kw = dict(kw, active=alloc, **(dict(device=device) if gpu else {}))
    plain = run(*head, first, count, *tail, **kw)
    masked = run(*head, first, count, *(tail if tail_masked is None else tail_masked), mask=mask, **kw)

    def of_pair(prof, i):
        # (RxProfile's arrays begin with the pair axis, the others' with the point or track axis)
        # (a one-dimensional field -- the scales of RxProfileSoft -- belongs to every pair)
        return type(prof)(*(a[i] if type(prof) is R.RxProfile else a if a.ndim == 1 else a[:, i] for a in prof[:-1]), prof.decisions)
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def run_sim_mc(system, n_fft, cp, w_tx, w_rx, channels, snr_db, ensemble, bits_per_subcar=4,
               symbols_per_tx=16, tail_tx=None, tail_rx=None, roll_off=ROLL_OFF, seed=0, device=0,
               frame_range=None):
    """``run_sim_mc`` (lines 334-360) for every (window pair, SNR, channel) at once.

    w_tx [pairs][P], w_rx [pairs][N+delta].  Returns (counts_masked, counts_plain), uint64
    [pairs][n_snr][n_channels][4]; BER = counts[..., 0] / counts[..., 1]."""
    st = V.make_structure(system, n_fft, cp, tail_tx, tail_rx)
    w_tx, w_rx = np.atleast_2d(w_tx), np.atleast_2d(w_rx)
    h = np.atleast_2d(np.asarray(channels))
    snr = np.atleast_1d(np.asarray(snr_db, dtype=np.float64))
    cfg = S.make_cfg(st, bits_per_subcar, symbols_per_tx, h.shape[1], h.shape[0], snr.size,
                     w_tx.shape[0], noise_before_truncate=True, seed=seed)
    lo, n = _frames(ensemble, frame_range)
    with S.Plan(cfg, w_tx, w_rx, h.astype(np.complex64), snr.astype(np.float32), device=device) as plan:
        plan.set_allocation(half_band_allocation(n_fft))
        plain = plan.run(lo, n)
        plan.set_tx_mask(tx_mask(st.sym_len, roll_off))
        # fresh frames: the reference draws new noise for the masked run (line 352)
        masked = plan.run(ensemble + lo, n)
    return masked, plain


def ber_for_window_file(type_ofdm, cp, windows, channels, snr_db, num_subcar=256, bits_per_subcar=4,
                        symbols_per_tx=16, ensemble=100, tail_tx=8, tail_rx=10, seed=0, device=0,
                        frame_range=None):
    """Loop nest of lines 56-263 for one window file: every window pair of the file + the RC
    pair, plain and masked.  Returns ({variable name: BER vs SNR}, (counts_masked, counts_plain))
    with the saved variable names of lines 287-330 (``berSNR``, ``berMaskedSNR``, ``berRCSNR``,
    ``berMaskedRCSNR``, ``ber[Masked]SNRStep{1,2,3}{A,B}``)."""
    st, plan, w_tx, w_rx, _, _ = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx)
    names = [n for n, _ in plan]
    masked, plain = run_sim_mc(type_ofdm, num_subcar, cp, w_tx, w_rx, channels, snr_db, ensemble,
                               bits_per_subcar, symbols_per_tx, st.tail_tx, st.tail_rx, seed=seed,
                               device=device, frame_range=frame_range)
    return results_from_counts(names, masked, plain), (masked, plain)


def spectrum_for_window_file(type_ofdm, cp, windows, num_subcar=256, symbols=None, rng=None, roll_off=ROLL_OFF,
                             gpu=True, device=0, tail_tx=8, tail_rx=10):
    """Spectrum companion of ``ber_for_window_file``: what the mask buys.  Every window pair of the file
    + the RC pair, half-band loading, 256 symbols of 16-QAM (``timefreq.draw_symbols``' draw on the loaded
    bins; or ``symbols`` [N/2, S]); per pair the averaged periodogram [8N] of the plain and of the masked
    waveform, all of them in ONE ``wofdm_tx_psd_batch_masked`` call (gpu=False: the fp64 host mirror
    ``timefreq.tx_waveform`` + ``psd_estimate``).  OBR = mean of the periodogram over the bins of the 8N grid
    that belong to unloaded subcarriers (bin f to subcarrier f // 8: ``estimate_obr``'s figure with the
    allocation in place of the guard band).  Returns {name: {"psd", "psd_masked", "obr", "obr_masked",
    "f_axis"}} with the names of ``V.matlab_pair_plan``."""
    from . import timefreq as T
    n = num_subcar
    st, plan, wins, _, alloc, mask = _window_file_setup(type_ofdm, cp, windows, n, tail_tx, tail_rx, roll_off, rx=False)
    if symbols is None:
        rng = np.random.RandomState() if rng is None else rng
        symbols = rng.choice(T.SYMBOLS_16QAM, size=(int(alloc.sum()), T.NO_SYMBOLS), replace=True)
    symbols = np.asarray(symbols)
    grid = np.zeros((n, symbols.shape[1]), dtype=np.complex128)
    grid[alloc] = symbols
    overlap = st.tail_tx
    fft_len = 8 * n
    if gpu:
        jobs = []
        for w in wins:
            jobs += [(0, st.cp, st.cs, overlap, w), (0, st.cp, st.cs, overlap, w, mask)]
        ests = T.tx_psd_batch_gpu(n, grid.T.astype(np.complex64)[None], jobs, device)
    else:
        ests = [T.psd_estimate(T.tx_waveform(st, grid, w, overlap, m, guard_band=None), fft_len)
                for w in wins for m in (None, mask)]
    unloaded = np.fft.fftshift(np.repeat(~alloc, fft_len // n))
    f_axis = np.linspace(-.5, .5 - 1 / fft_len, fft_len) / 200e-9
    out = {}
    for i, (name, _) in enumerate(plan):
        plain, masked = np.asarray(ests[2 * i]), np.asarray(ests[2 * i + 1])
        out[name] = {"psd": plain, "psd_masked": masked, "obr": plain[unloaded].mean(),
                     "obr_masked": masked[unloaded].mean(), "f_axis": f_axis}
    return out


def interference_for_window_file(type_ofdm, cp, windows, channels, num_subcar=256, roll_off=ROLL_OFF, gpu=True,
                                 device=0, tail_tx=8, tail_rx=10):
    """Interference companion of ``ber_for_window_file`` and ``spectrum_for_window_file``: what the mask costs.
    Every window pair of the file + the RC pair under half-band loading, for every channel [n_channels][taps]:
    the closed-form ICI + ISI power per subcarrier and the wanted power |A_0[n, n]|^2, plain and masked -- on the
    GPU two ``wofdm_interference_masked`` calls over all pairs and channels (one with the mask, one with the
    allocation alone; gpu=False: the fp64 host mirror ``interference.interf_power_masked``).  Returns {name:
    {"power", "power_masked", "wanted", "wanted_masked"}}, each [n_channels][N], with the names of
    ``V.matlab_pair_plan``; SIR per subcarrier = wanted / power on the loaded bins (both are 0 on the others)."""
    from . import interference as I
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    h = np.atleast_2d(np.asarray(channels))
    if gpu:
        plain = I.interf_power_masked_gpu(st, w_tx, w_rx, h, active=alloc, device=device)
        masked = I.interf_power_masked_gpu(st, w_tx, w_rx, h, active=alloc, mask=mask, device=device)
    else:
        def host(m):
            res = [[I.interf_power_masked(st, wt, wr, hc, active=alloc, mask=m) for hc in h]
                   for wt, wr in zip(w_tx, w_rx)]
            return (np.array([[r[0] for r in row] for row in res]), np.array([[r[1] for r in row] for row in res]))
        plain, masked = host(None), host(mask)
    return {name: {"power": plain[0][i], "wanted": plain[1][i], "power_masked": masked[0][i],
                   "wanted_masked": masked[1][i]} for i, (name, _) in enumerate(plan)}


def papr_for_window_file(type_ofdm, cp, windows, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16, ensemble=1000,
                         roll_off=ROLL_OFF, lo_db=0.0, step_db=0.25, n_bins=64, seed=0, frame_range=None, gpu=True,
                         device=0, tail_tx=8, tail_rx=10):
    """PAPR companion of ``ber_for_window_file``, ``spectrum_for_window_file`` and ``interference_for_window_file``: what
    the mask and the window do to the envelope.  Every window pair of the file + the RC pair under half-band loading; per
    pair the PAPR histogram of the symbol periods of the frames its BER cell transmits (``ensemble`` frames of
    ``symbols_per_tx`` symbols, or ``frame_range`` = (first, count); same seed -> same frames as a plan with one SNR point
    and one channel), plain and masked (``tx_mask(P)``) -- on the GPU two ``wofdm_tx_papr`` calls over all pairs (one
    with the mask, one with the allocation alone; gpu=False: the fp64 host mirror ``timefreq.frame_papr`` on random
    symbols of its own draw, for small ensembles).  Returns {name: {"hist", "hist_masked", "ccdf", "ccdf_masked",
    "max_db", "max_db_masked", "edges_db"}} with the names of ``V.matlab_pair_plan``; ccdf[i] = Pr(PAPR >= edges_db[i])."""
    from . import timefreq as T
    n = num_subcar
    st, plan, w_tx, _, alloc, mask = _window_file_setup(type_ofdm, cp, windows, n, tail_tx, tail_rx, roll_off, rx=False)
    first, count = _frames(ensemble, frame_range)
    if gpu:
        plain = T.tx_papr_gpu(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, lo_db=lo_db,
                              step_db=step_db, n_bins=n_bins, device=device)
        masked = T.tx_papr_gpu(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=mask,
                               lo_db=lo_db, step_db=step_db, n_bins=n_bins, device=device)
    else:
        rs = np.random.RandomState(seed)
        tab = T.qam_table(bits_per_subcar)
        B = st.sym_len - st.tail_tx

        def host(m):
            hists, peaks = [], []
            for w in w_tx:
                grids = tab[rs.randint(0, tab.size, size=(count, symbols_per_tx, n))] * alloc[None, None, :]
                per = T.frame_papr(st, grids, w, m)
                hists.append(T.papr_hist(per, B, lo_db, step_db, n_bins))
                peaks.append((B * per[..., 0] / per[..., 1]).max())
            return np.stack(hists), np.asarray(peaks)
        plain, masked = host(None), host(mask)
    edges = lo_db + step_db * np.arange(n_bins)
    with np.errstate(divide="ignore"):
        db = [10.0 * np.log10(np.asarray(r[1], dtype=np.float64)) for r in (plain, masked)]
    return {name: {"hist": plain[0][i], "hist_masked": masked[0][i], "ccdf": T.papr_ccdf(plain[0][i]),
                   "ccdf_masked": T.papr_ccdf(masked[0][i]), "max_db": db[0][i], "max_db_masked": db[1][i],
                   "edges_db": edges} for i, (name, _) in enumerate(plan)}


def profile_for_window_file(type_ofdm, cp, windows, channels, snr_db, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                            ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8,
                            tail_rx=10):
    """Per-subcarrier companion of ``ber_for_window_file``: where in the band the errors sit.  Every window pair of the
    file + the RC pair under half-band loading, for every SNR point and channel [n_channels][taps]: bit errors, symbol
    errors and error power sum |Xhat - X|^2 per subcarrier of the frames the BER cells run (``ensemble`` frames, or
    ``frame_range`` = (first, count); same seed -> the frames of a plan with the same pairs, SNR points and channels),
    plain and masked (``tx_mask(P)``) -- on the GPU two ``wofdm_rx_profile`` calls (gpu=False: the fp64 host route
    ``rx_profile.rx_profile_host`` on the same Philox streams, for small ensembles).  Unlike ``run_sim_mc`` both runs
    cover the SAME frame range: bits and noise are those of the cell, so the two profiles differ by the mask alone.
    Returns {name: {"profile", "profile_masked"}} with the names of ``V.matlab_pair_plan``; each is an
    ``rx_profile.RxProfile`` of that pair, arrays [n_snr, n_channels, N] (``rx_profile.ber_per_bin``, ``evm_db``)."""
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    return _profiles_per_pair("", plan, alloc, mask, head, ensemble, frame_range, gpu, device)


def aci_for_window_file(type_ofdm, cp, windows, channels, snr_db, delays, level_db=0.0, aci_channels=None, num_subcar=256,
                        bits_per_subcar=4, symbols_per_tx=16, ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None,
                        gpu=True, device=0, tail_tx=8, tail_rx=10):
    """The neighbour's side of the mask experiment: ``profile_for_window_file`` with a second transmitter of the same
    numerology on the COMPLEMENTARY half band, not symbol-aligned with the victim -- what the free half band and the
    confined spectrum are for, and what the Rx window is there to reject.  Every window pair of the file + the RC pair, the
    victim on ``half_band_allocation``, the neighbour on the other bins with the pair's Tx window (and the mask, in the masked
    run), ``level_db`` dB against the victim, through ``aci_channels`` [n_channels][taps] (None: the victim's), its symbols
    beginning ``delay`` samples after the victim's for every delay of ``delays`` (0 <= delay < stride).  ``snr_db`` is the
    victim's SNR; the neighbour comes on top.  On the GPU two ``wofdm_rx_profile_aci`` calls per delay (gpu=False: the fp64
    host route ``rx_profile.rx_profile_aci_host``, for small ensembles); the frames are those of ``profile_for_window_file``
    with the same arguments, so the two results differ by the neighbour alone.
    Returns {name: {delay: {"profile", "profile_masked"}}} with the names of ``V.matlab_pair_plan``; each an
    ``rx_profile.RxProfile`` of that pair, arrays [n_snr, n_channels, N]."""
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    out = {name: {} for name, _ in plan}
    for d in delays:
        per_pair = _profiles_per_pair("_aci", plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(~alloc, int(d)),
                                      aci_level_db=level_db, aci_h=aci_channels)
        for name, _ in plan:
            out[name][int(d)] = per_pair[name]
    return out


def sync_for_window_file(type_ofdm, cp, windows, channels, snr_db, points, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                         ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """The synchronisation side of the mask experiment: ``profile_for_window_file`` with a receiver whose windows begin early
    or late and whose oscillator is off -- the tolerance the cyclic suffix, the prefix removal and the Rx window trade, and
    where the window pairs differ most.  Every window pair of the file + the RC pair under half-band loading, for every SNR
    point, channel and point of ``points`` (``rx_profile.SyncPoint`` or (timing, cfo, cfo_tracked) tuples: samples, subcarrier
    spacings, 0 / 1), plain and masked (``tx_mask(P)``) -- on the GPU two ``wofdm_rx_profile_sync`` calls whatever
    len(points) is: the Tx chain and the power pass of a frame run once for all its points (gpu=False: the fp64 host route
    ``rx_profile.rx_profile_sync_host``, for small ensembles).  The frames are those of ``profile_for_window_file`` with the
    same arguments, so the point (0, 0) is its result.
    Returns {name: {"profile", "profile_masked"}} with the names of ``V.matlab_pair_plan``; each an
    ``rx_profile.RxProfileSync`` of that pair, arrays [points, n_snr, n_channels, N] and [points, n_snr, n_channels, S - 1]."""
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    return _profiles_per_pair("_sync", plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(list(points),))


def pn_for_window_file(type_ofdm, cp, windows, channels, snr_db, points, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                       ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """The oscillator side of the mask experiment: ``profile_for_window_file`` with a receiver whose oscillator phase is a
    random walk -- a common phase error that grows with the distance from the pilot, and ICI, which the Rx window is there to
    reject and in which the window pairs differ.  Every window pair of the file + the RC pair under half-band loading, for
    every SNR point, channel and point of ``points`` (``rx_profile.PnPoint`` or (linewidth, cpe_tracked) tuples: subcarrier
    spacings, 0 / 1), plain and masked (``tx_mask(P)``) -- on the GPU two ``wofdm_rx_profile_pn`` calls whatever len(points)
    is: the Tx chain, the power pass and the phase walk of a frame run once for all its points (gpu=False: the fp64 host
    route ``rx_profile.rx_profile_pn_host``, for small ensembles).  The frames are those of ``profile_for_window_file`` with
    the same arguments, so a point of linewidth 0 is its result.
    Returns {name: {"profile", "profile_masked"}} with the names of ``V.matlab_pair_plan``; each an
    ``rx_profile.RxProfileSync`` of that pair, arrays [points, n_snr, n_channels, N] and [points, n_snr, n_channels, S - 1]."""
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    return _profiles_per_pair("_pn", plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(list(points),))


def doppler_for_window_file(type_ofdm, cp, windows, tracks, knot_step, snr_db, num_subcar=256, bits_per_subcar=4,
                            symbols_per_tx=16, ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0,
                            tail_tx=8, tail_rx=10):
    """The mobility side of the mask experiment: ``profile_for_window_file`` over channels that move within the frame, under
    a receiver that equalises with the pilot of symbol 0 alone -- where both the Rx window (ICI rejection) and the distance
    from the pilot matter.  Every window pair of the file + the RC pair under half-band loading, for every SNR point, channel
    and track of ``tracks`` [n_tracks, n_channels, n_knots, taps] (``channels.gen_channel_tracks``: the same realisations at
    several speeds; knot q at on-air index q * knot_step), plain and masked (``tx_mask(P)``) -- on the GPU two
    ``wofdm_rx_profile_doppler`` calls whatever the number of tracks: the Tx chain of a frame runs once for all of them
    (gpu=False: the fp64 host route ``rx_profile.rx_profile_doppler_host``, for small ensembles).  The frames are those of
    ``profile_for_window_file`` with the same arguments, so a track whose knots all equal its channel is that result.
    Returns {name: {"profile", "profile_masked"}} with the names of ``V.matlab_pair_plan``; each an
    ``rx_profile.RxProfileSync`` of that pair, arrays [tracks, n_snr, n_channels, N] and [tracks, n_snr, n_channels, S - 1]."""
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.asarray(tracks), knot_step, snr_db, seed)
    return _profiles_per_pair("_doppler", plan, alloc, mask, head, ensemble, frame_range, gpu, device)


def pa_for_window_file(type_ofdm, cp, windows, channels, snr_db, points, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                       ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, symbols=None, rng=None, gpu=True, device=0,
                       tail_tx=8, tail_rx=10):
    """The amplifier's side of the mask experiment: what the PAPR of ``papr_for_window_file`` costs behind the transmitter's
    last stage -- "which window pair is best at 3 dB back-off".  Every window pair of the file + the RC pair under half-band
    loading, plain and masked (``tx_mask(P)``), for every point of ``points`` (``rx_profile.PaPoint`` or (model, ibo_db, smooth)
    tuples: linear, Rapp, soft limiter): the receive profile of ``profile_for_window_file`` behind the amplifier, per SNR point
    and channel, and the periodogram and out-of-band radiation of ``spectrum_for_window_file`` behind it (``symbols`` / ``rng``
    as there) -- compression raises the error vector on the loaded bins and puts back, as regrowth, the radiation window and
    mask removed.  On the GPU two ``wofdm_rx_profile_pa`` calls and one ``wofdm_tx_psd_batch_pa`` call whatever len(points) is
    (and the two ``wofdm_tx_papr`` runs of ``rx_profile.pa_ref_power``, which measure the mean power per pair the receive
    route's back-off counts from; the spectrum route measures each waveform's own); gpu=False: the fp64 host routes
    ``rx_profile.rx_profile_pa_host`` and ``timefreq.tx_waveform(..., pa=)``, for small ensembles.  The frames are those of
    ``profile_for_window_file`` with the same arguments, so a ``PA_LINEAR`` point is its result.
    Returns {name: {"profile", "profile_masked", "psd", "psd_masked", "obr", "obr_masked", "ref_power", "ref_power_masked",
    "f_axis"}} with the names of ``V.matlab_pair_plan``: the profiles ``rx_profile.RxProfilePa`` of that pair, arrays [points,
    n_snr, n_channels, ...]; psd [points, 8 N], obr [points]."""
    from . import rx_profile as R
    from . import timefreq as T
    n = num_subcar
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, n, tail_tx, tail_rx, roll_off)
    pts = [R._pa_point(q) for q in points]
    first, count = _frames(ensemble, frame_range)
    # the receive route: the mean power per pair, then one call per system
    ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                          **(dict(device=device) if gpu else {})) for m in (None, mask)]
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    out = _profiles_per_pair("_pa", plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(pts, ref[0]),
                             tail_masked=(pts, ref[1]))
    # the spectrum route: every (pair, system, point) as one job
    if symbols is None:
        rng = np.random.RandomState() if rng is None else rng
        symbols = rng.choice(T.SYMBOLS_16QAM, size=(int(alloc.sum()), T.NO_SYMBOLS), replace=True)
    grid = np.zeros((n, np.asarray(symbols).shape[1]), dtype=np.complex128)
    grid[alloc] = np.asarray(symbols)
    fft_len = 8 * n
    combos = [(w, m, q) for w in w_tx for m in (None, mask) for q in pts]
    if gpu:
        ests = T.tx_psd_batch_gpu(n, grid.T.astype(np.complex64)[None], [(0, st.cp, st.cs, st.tail_tx, w, m, q) for w, m, q in combos],
                                  device)
    else:
        ests = [T.psd_estimate(T.tx_waveform(st, grid, w, st.tail_tx, m, guard_band=None, pa=q), fft_len) for w, m, q in combos]
    ests = np.asarray(ests).reshape(len(plan), 2, len(pts), fft_len)
    unloaded = np.fft.fftshift(np.repeat(~alloc, fft_len // n))
    f_axis = np.linspace(-.5, .5 - 1 / fft_len, fft_len) / 200e-9
    for i, (name, _) in enumerate(plan):
        out[name].update({"psd": ests[i, 0], "psd_masked": ests[i, 1], "obr": ests[i, 0][:, unloaded].mean(axis=1),
                          "obr_masked": ests[i, 1][:, unloaded].mean(axis=1), "ref_power": ref[0][i],
                          "ref_power_masked": ref[1][i], "f_axis": f_axis})
    return out


def link_for_window_file(type_ofdm, cp, windows, channels, snr_db, points, tracks=None, knot_step=None, aci_channels=None,
                         num_subcar=256, bits_per_subcar=4, symbols_per_tx=16, ensemble=100, roll_off=ROLL_OFF, seed=0,
                         frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """The whole link of the mask experiment: ``profile_for_window_file`` with the impairments of ``pa_for_window_file``,
    ``doppler_for_window_file``, ``aci_for_window_file``, ``sync_for_window_file`` and ``pn_for_window_file`` in ONE chain -- "which
    window pair is best at 3 dB back-off, 100 km/h, a 1e-3 linewidth and a neighbour 10 dB up"; the effects do not add.  Every
    window pair of the file + the RC pair under half-band loading, for every SNR point, channel and point of ``points``
    (``rx_profile.LinkPoint`` or tuples in its order, each switching on any subset), plain and masked (``tx_mask(P)``): the
    amplifier's back-off counts from ``rx_profile.pa_ref_power`` of the pair (measured only where a point has an amplifier),
    ``tracks`` [n_tracks, n_channels, n_knots, taps] and ``knot_step`` as in ``doppler_for_window_file``, the neighbour on the
    complementary half band through ``aci_channels`` (None: the victim's) as in ``aci_for_window_file``.  On the GPU two
    ``wofdm_rx_profile_link`` calls whatever len(points) is (gpu=False: the fp64 host route
    ``rx_profile.rx_profile_link_host``, for small ensembles).  The frames are those of ``profile_for_window_file`` with the
    same arguments, so an all-off point is its result.
    Returns {name: {"profile", "profile_masked"}} with the names of ``V.matlab_pair_plan``; each an
    ``rx_profile.RxProfileLink`` of that pair, arrays [points, n_snr, n_channels, ...]."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    side = (tracks, knot_step, ~alloc if any(q.aci is not None for q in pts) else None, aci_channels)
    return _profiles_per_pair("_link", plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(pts, *side, ref[0]),
                              tail_masked=(pts, *side, ref[1]))


def soft_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, scales=None, tracks=None, knot_step=None,
                         aci_channels=None, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16, ensemble=100, roll_off=ROLL_OFF,
                         seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``link_for_window_file`` with soft decisions: the same pairs, frames, points (None: one all-off point) and side arguments,
    and for the scales ``scales`` (None: ``rx_profile.SOFT_SCALES``) the penalties from which ``rx_profile.gmi_per_bin``,
    ``gmi_per_symbol`` and ``gmi`` form the rate a coded receiver could carry -- what ranks window pairs where the uncoded error
    rates are far above anything a link runs at.  On the GPU two ``wofdm_rx_profile_soft`` calls whatever the number of points
    and scales (gpu=False: ``rx_profile.rx_profile_soft_host``).  Returns {name: {"profile", "profile_masked"}}, each an
    ``rx_profile.RxProfileSoft`` of that pair, arrays [points, n_snr, n_channels, ...]; its hard fields are
    ``link_for_window_file``'s."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed)
    side = (tracks, knot_step, ~alloc if any(q.aci is not None for q in pts) else None, aci_channels)
    return _profiles_per_pair("_soft", plan, alloc, mask, head, ensemble, frame_range, gpu, device, tail=(pts, scales, *side, ref[0]),
                              tail_masked=(pts, scales, *side, ref[1]))


def tracking_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, tracking=None, pilot_spacing=8, scales=None,
                             tracks=None, knot_step=None, aci_channels=None, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                             ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``soft_for_window_file`` behind a receiver that tracks -- which window pair is best once the common rotation is estimated
    and removed and the channel estimate follows the frame: the same pairs, frames, points and side arguments, a comb of pilots
    on every ``pilot_spacing``-th loaded bin (``rx_profile.pilot_comb``; None: no comb) and one ``rx_profile.TrackingPoint`` (or
    (cpe, post)) per point in ``tracking`` (None: all (0, 0)).  On the GPU two ``wofdm_rx_profile_tracking`` calls whatever the
    number of points and scales (gpu=False: ``rx_profile.rx_profile_tracking_host``).  Returns {name: {"profile",
    "profile_masked"}}, each an ``rx_profile.RxProfileTracking`` of that pair, arrays [points, n_snr, n_channels, ...]; with no
    comb and every point (0, 0) its fields are ``soft_for_window_file``'s."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    pil = None if pilot_spacing is None else R.pilot_comb(alloc, pilot_spacing)
    run = R.rx_profile_tracking_gpu if gpu else R.rx_profile_tracking_host
    side = dict(tracks=tracks, knot_step=knot_step, aci_active=~alloc if any(q.aci is not None for q in pts) else None,
                aci_h=aci_channels, active=alloc, **(dict(device=device) if gpu else {}))
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed, first, count, pts,
            tracking, pil, scales)
    plain, masked = run(*head, ref_power=ref[0], **side), run(*head, ref_power=ref[1], mask=mask, **side)

    def of_pair(prof, i):
        # (the sums begin with the point axis, then the pair's; the scales and the decisions belong to every pair)
        return type(prof)(*(a[:, i] for a in prof[:-3]), *prof[-3:])
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def coded_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, tracking=None, pilot_spacing=8, scales=None,
                          llr_scale=None, interleave=True, codes=(0, 1, 2), tracks=None, knot_step=None, aci_channels=None,
                          num_subcar=256, bits_per_subcar=4, symbols_per_tx=16, ensemble=100, roll_off=ROLL_OFF, seed=0,
                          frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``tracking_for_window_file`` with the coded link behind it -- the coded BER of every window pair at the rates ``codes``
    (indices of ``rx_profile.CODE_RATES``): the same pairs, frames, points, comb and receivers, the demapper's soft bits
    quantised with ``llr_scale`` (None: ``rx_profile.LLR_SCALE``), interleaved with ``rx_profile.default_interleaver``
    (interleave=False: not at all) and decoded per data symbol.  On the GPU two ``wofdm_rx_profile_coded`` calls (gpu=False:
    ``rx_profile.rx_profile_coded_host``).  Returns {name: {"profile", "profile_masked"}}, each an ``rx_profile.RxProfileCoded``
    of that pair, arrays [points, n_snr, n_channels, ...], without soft bits."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    pil = None if pilot_spacing is None else R.pilot_comb(alloc, pilot_spacing)
    n_c = int(bits_per_subcar) * int((alloc & ~pil).sum() if pil is not None else alloc.sum())
    run = R.rx_profile_coded_gpu if gpu else R.rx_profile_coded_host
    side = dict(tracks=tracks, knot_step=knot_step, aci_active=~alloc if any(q.aci is not None for q in pts) else None,
                aci_h=aci_channels, active=alloc, **(dict(device=device) if gpu else {}))
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed, first, count, pts,
            tracking, pil, scales, R.LLR_SCALE if llr_scale is None else llr_scale, R.default_interleaver(n_c) if interleave else None,
            codes)
    plain, masked = run(*head, ref_power=ref[0], **side), run(*head, ref_power=ref[1], mask=mask, **side)
    n = len(R.RxProfileTracking._fields)

    def of_pair(prof, i):
        # (the tracking sums, then the scales and the decisions; the code errors; what belongs to every pair)
        return type(prof)(*(a[:, i] for a in prof[:n - 3]), *prof[n - 3:n], prof.info_err[:, i], prof.cw_err[:, i], *prof[n + 2:])
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def coded_frame_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, tracking=None, pilot_spacing=8, scales=None,
                                llr_scale=None, interleave=True, codes=(0, 1, 2), sym_rot=None, tracks=None, knot_step=None,
                                aci_channels=None, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16, ensemble=100,
                                roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``coded_for_window_file`` with ONE codeword per frame over its data symbols in the place of one per symbol: the same pairs,
    frames, points, comb, receivers and soft bits, interleaved by ``rx_profile.frame_interleaver`` -- within a symbol
    ``rx_profile.default_interleaver`` (interleave=False: not at all), from symbol to symbol rotated by ``sym_rot`` (None:
    ``rx_profile.default_sym_rot``).  On the GPU two ``wofdm_rx_profile_coded_frame`` calls (gpu=False:
    ``rx_profile.rx_profile_coded_frame_host``).  Returns {name: {"profile", "profile_masked"}}, each an
    ``rx_profile.RxProfileCodedFrame`` of that pair, arrays [points, n_snr, n_channels, ...], without soft bits."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    pil = None if pilot_spacing is None else R.pilot_comb(alloc, pilot_spacing)
    n_c = int(bits_per_subcar) * int((alloc & ~pil).sum() if pil is not None else alloc.sum())
    run = R.rx_profile_coded_frame_gpu if gpu else R.rx_profile_coded_frame_host
    side = dict(tracks=tracks, knot_step=knot_step, aci_active=~alloc if any(q.aci is not None for q in pts) else None,
                aci_h=aci_channels, active=alloc, **(dict(device=device) if gpu else {}))
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed, first, count, pts,
            tracking, pil, scales, R.LLR_SCALE if llr_scale is None else llr_scale, R.default_interleaver(n_c) if interleave else None,
            codes, sym_rot)
    plain, masked = run(*head, ref_power=ref[0], **side), run(*head, ref_power=ref[1], mask=mask, **side)
    n = len(R.RxProfileTracking._fields)

    def of_pair(prof, i):
        # (the tracking sums, then the scales and the decisions; the code errors; what belongs to every pair)
        return type(prof)(*(a[:, i] for a in prof[:n - 3]), *prof[n - 3:n], prof.info_err[:, i], prof.cw_err[:, i], *prof[n + 2:])
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def ldpc_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, tracking=None, pilot_spacing=8, scales=None,
                         llr_scale=None, interleave=True, codes=((4, 8), (4, 12), (4, 16)), sym_rot=None, tracks=None, knot_step=None,
                         aci_channels=None, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16, ensemble=100,
                         roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``coded_frame_for_window_file`` with quasi-cyclic LDPC codewords over the frame in the place of the convolutional one: the
    same pairs, frames, points, comb, receivers, soft bits and frame interleaver; ``codes`` are (J, L) or (J, L, max_iter) each
    (``rx_profile.ldpc_lift``).  On the GPU two ``wofdm_rx_profile_ldpc`` calls (gpu=False: ``rx_profile.rx_profile_ldpc_host``).
    Returns {name: {"profile", "profile_masked"}}, each an ``rx_profile.RxProfileLdpc`` of that pair, arrays [points, n_snr,
    n_channels, ...], without soft bits."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    pil = None if pilot_spacing is None else R.pilot_comb(alloc, pilot_spacing)
    n_c = int(bits_per_subcar) * int((alloc & ~pil).sum() if pil is not None else alloc.sum())
    run = R.rx_profile_ldpc_gpu if gpu else R.rx_profile_ldpc_host
    side = dict(tracks=tracks, knot_step=knot_step, aci_active=~alloc if any(q.aci is not None for q in pts) else None,
                aci_h=aci_channels, active=alloc, **(dict(device=device) if gpu else {}))
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed, first, count, pts,
            tracking, pil, scales, R.LLR_SCALE if llr_scale is None else llr_scale, R.default_interleaver(n_c) if interleave else None,
            codes, sym_rot)
    plain, masked = run(*head, ref_power=ref[0], **side), run(*head, ref_power=ref[1], mask=mask, **side)
    n = len(R.RxProfileTracking._fields)

    def of_pair(prof, i):
        # (the tracking sums, then the scales and the decisions; the four code counters; what belongs to every pair)
        return type(prof)(*(a[:, i] for a in prof[:n - 3]), *prof[n - 3:n], *(a[:, i] for a in prof[n:n + 4]), *prof[n + 4:])
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def coset_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, tracking=None, pilot_spacing=8, scales=None,
                          llr_scale=None, interleave=True, codes=(0, 1, 2), ldpc_codes=((4, 8), (4, 12), (4, 16)), sym_rot=None,
                          tracks=None, knot_step=None, aci_channels=None, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                          ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``coded_frame_for_window_file`` and ``ldpc_for_window_file`` in one, against random transmitted words in the place of the
    all-zero one: the same pairs, frames, points, comb, receivers, soft bits and frame interleaver, the Viterbi rates ``codes`` and
    the LDPC codes ``ldpc_codes`` (an empty sequence switches a family off) behind one receive chain.  On the GPU two
    ``wofdm_rx_profile_coset`` calls (gpu=False: ``rx_profile.rx_profile_coset_host``).  Returns {name: {"profile",
    "profile_masked"}}, each an ``rx_profile.RxProfileCoset`` of that pair, arrays [points, n_snr, n_channels, ...], without soft
    bits."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    pil = None if pilot_spacing is None else R.pilot_comb(alloc, pilot_spacing)
    n_c = int(bits_per_subcar) * int((alloc & ~pil).sum() if pil is not None else alloc.sum())
    run = R.rx_profile_coset_gpu if gpu else R.rx_profile_coset_host
    side = dict(tracks=tracks, knot_step=knot_step, aci_active=~alloc if any(q.aci is not None for q in pts) else None,
                aci_h=aci_channels, active=alloc, **(dict(device=device) if gpu else {}))
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed, first, count, pts,
            tracking, pil, scales, R.LLR_SCALE if llr_scale is None else llr_scale, R.default_interleaver(n_c) if interleave else None,
            codes, ldpc_codes, sym_rot)
    plain, masked = run(*head, ref_power=ref[0], **side), run(*head, ref_power=ref[1], mask=mask, **side)
    n = len(R.RxProfileTracking._fields)
    per_pair = ("info_err", "cw_err", "ldpc_info_err", "ldpc_cw_err", "unconverged", "iterations")

    def of_pair(prof, i):
        # (the tracking sums, then the scales and the decisions; the code counters; what belongs to every pair)
        return prof._replace(**{f: getattr(prof, f)[:, i] for f in prof._fields[:n - 3] + per_pair})
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def harq_for_window_file(type_ofdm, cp, windows, channels, snr_db, points=None, tracking=None, pilot_spacing=8, scales=None,
                         llr_scale=None, interleave=True, ldpc_codes=((4, 8), (4, 12), (4, 16)), sym_rot=None, rounds=4, combine=True,
                         tracks=None, knot_step=None, aci_channels=None, num_subcar=256, bits_per_subcar=4, symbols_per_tx=16,
                         ensemble=100, roll_off=ROLL_OFF, seed=0, frame_range=None, gpu=True, device=0, tail_tx=8, tail_rx=10):
    """``coset_for_window_file``'s pairs, frames, points, comb, receivers, soft bits and frame interleaver with retransmissions: the
    frames of a cell in groups of ``rounds`` transmissions of the same LDPC words, combined (``combine``) and decoded until the
    syndrome vanishes; the frames' number and the first frame must be multiples of ``rounds``.  On the GPU two
    ``wofdm_rx_profile_harq`` calls, plain and masked (gpu=False: ``rx_profile.rx_profile_harq_host``).  Returns {name: {"profile",
    "profile_masked"}}, each an ``rx_profile.RxProfileHarq`` of that pair, arrays [points, n_snr, n_channels, ...], without soft
    bits -- ``rx_profile.harq_goodput`` and ``harq_bits_per_sample`` (with ``symbols_per_tx`` and the structure's stride) are the
    figures the pairs compare by."""
    from . import rx_profile as R
    st, plan, w_tx, w_rx, alloc, mask = _window_file_setup(type_ofdm, cp, windows, num_subcar, tail_tx, tail_rx, roll_off)
    pts = [R.LinkPoint()] if points is None else [R.LinkPoint(*q) for q in points]
    first, count = _frames(ensemble, frame_range)
    ref = [None, None]
    if any(q.pa is not None for q in pts):
        ref = [R.pa_ref_power(st, bits_per_subcar, symbols_per_tx, w_tx, seed, first, count, active=alloc, mask=m, gpu=gpu,
                              **(dict(device=device) if gpu else {})) for m in (None, mask)]
    pil = None if pilot_spacing is None else R.pilot_comb(alloc, pilot_spacing)
    n_c = int(bits_per_subcar) * int((alloc & ~pil).sum() if pil is not None else alloc.sum())
    run = R.rx_profile_harq_gpu if gpu else R.rx_profile_harq_host
    side = dict(tracks=tracks, knot_step=knot_step, aci_active=~alloc if any(q.aci is not None for q in pts) else None,
                aci_h=aci_channels, active=alloc, **(dict(device=device) if gpu else {}))
    head = (st, bits_per_subcar, symbols_per_tx, w_tx, w_rx, np.atleast_2d(np.asarray(channels)), snr_db, seed, first, count, pts,
            tracking, pil, scales, R.LLR_SCALE if llr_scale is None else llr_scale, R.default_interleaver(n_c) if interleave else None,
            ldpc_codes, sym_rot, rounds, combine)
    plain, masked = run(*head, ref_power=ref[0], **side), run(*head, ref_power=ref[1], mask=mask, **side)
    n = len(R.RxProfileTracking._fields)
    per_pair = ("acked", "unacked", "word_err", "undetected", "info_err", "iterations")

    def of_pair(prof, i):
        return prof._replace(**{f: getattr(prof, f)[:, i] for f in prof._fields[:n - 3] + per_pair})
    return {name: {"profile": of_pair(plain, i), "profile_masked": of_pair(masked, i)} for i, (name, _) in enumerate(plan)}


def results_from_counts(names, masked, plain):
    def ber(c):      # mean over channels of per-channel BER (lines 84-117)
        return (c[..., 0] / np.maximum(c[..., 1], 1)).mean(axis=-1)
    out = {}
    bm, bp = ber(masked), ber(plain)
    for i, name in enumerate(names):
        if name == "opt":
            out["berSNR"], out["berMaskedSNR"] = bp[i], bm[i]
        elif name == "rc":
            out["berRCSNR"], out["berMaskedRCSNR"] = bp[i], bm[i]
        else:
            out["berSNRStep" + name], out["berMaskedSNRStep" + name] = bp[i], bm[i]
    return out


def save_results(results_path, type_ofdm, cp, results):
    """Files of lines 118-125, 261-263 under ``ber_results/simulation_with_channel_mask``."""
    from scipy.io import savemat
    os.makedirs(results_path, exist_ok=True)
    base = "ber_%s_%dCP" % (type_ofdm, cp)
    groups = {"optimized_": [k for k in results if k == "berSNR" or k.startswith("berSNRStep")],
              "masked_optimized_": [k for k in results if k == "berMaskedSNR"
                                    or k.startswith("berMaskedSNRStep")],
              "rc_": ["berRCSNR"], "masked_rc_": ["berMaskedRCSNR"]}
    paths = []
    for prefix, keys in groups.items():
        keys = [k for k in keys if k in results]
        if keys:
            paths.append(os.path.join(results_path, prefix + base + ".mat"))
            savemat(paths[-1], {k: np.asarray(results[k]).reshape(-1, 1) for k in keys})
    return paths
