"""Per-subcarrier BER and EVM of the frames the BER loop runs (``wofdm_rx_profile``).

Where in the band the errors sit: for every cell (window pair, SNR, channel) and every subcarrier the bit errors, the
symbol errors and the error-vector power sum |Xhat - X|^2 over the decisions of the frames [frame_offset, frame_offset +
frames) -- the frames a ``Plan`` with the same cfg and seed simulates, so the bins add up to its counters.  The reference
reduces every frame to one BER (matlab/main_BER_calculation.m:272); for the half-band, spectrally masked system of
matlab/main_channel_mask.m the per-bin picture is the interesting one.

``rx_profile_gpu`` runs on the GPU (no CPU fallback); ``frame_profile`` is the fp64 numpy mirror of ONE frame with the
randomness given, ``rx_profile_host`` draws the same Philox streams on the host (csrc/philox.h) and runs it frame by frame
-- for small ensembles, the check of the GPU route.

``rx_profile_aci_gpu`` (``wofdm_rx_profile_aci``) is the same profile with an asynchronous adjacent-band neighbour on the
air -- the interference the Rx window is there to reject; ``frame_profile_aci`` and ``rx_profile_aci_host`` mirror it.

``rx_profile_sync_gpu`` (``wofdm_rx_profile_sync``) is the profile under receiver timing and carrier-frequency offset, a
list of ``SyncPoint`` per call, per subcarrier and per data symbol; ``frame_profile_sync`` and ``rx_profile_sync_host``
mirror it.

``rx_profile_doppler_gpu`` (``wofdm_rx_profile_doppler``) is the profile over channels that move within the frame, a list of
tracks (knots of the tap vector, linear in between) per call; ``tv_conv``, ``frame_profile_doppler`` and
``rx_profile_doppler_host`` mirror it.

``rx_profile_pa_gpu`` (``wofdm_rx_profile_pa``) is the profile behind a memoryless power amplifier (linear, Rapp, soft
limiter), a list of ``PaPoint`` per call, with the power before and behind the amplifier; ``pa_gain``, ``pa_apply``,
``frame_profile_pa`` and ``rx_profile_pa_host`` mirror it, ``pa_ref_power`` measures the mean power the back-off counts from.

``rx_profile_pn_gpu`` (``wofdm_rx_profile_pn``) is the profile under oscillator phase noise, the receiver's phase a random walk
drawn from Philox stream 3, a list of ``PnPoint`` (linewidth, free-running or common phase error tracked) per call;
``gen_pn_increments``, ``pn_walk``, ``frame_profile_pn`` and ``rx_profile_pn_host`` mirror it.

``rx_profile_link_gpu`` (``wofdm_rx_profile_link``) is the profile with all five combined in one chain, a list of ``LinkPoint``
per call, each switching on any subset; ``frame_profile_link`` and ``rx_profile_link_host`` mirror it, composed of the mirrors
above.

``rx_profile_soft_gpu`` (``wofdm_rx_profile_soft``) is the link call with soft decisions: beside the hard counters the max-log
bit metrics' penalties per bin and per data symbol for a list of scales, from which ``gmi_per_bin``, ``gmi_per_symbol`` and
``gmi`` form the achievable (BICM) rate; ``bit_llrs``, ``soft_penalties``, ``frame_profile_soft`` and ``rx_profile_soft_host``
mirror it.

``rx_profile_tracking_gpu`` (``wofdm_rx_profile_tracking``) is the soft call behind a receiver that tracks: a comb of pilot bins
(``pilot_comb``) gives a common-phase estimate per data symbol, a postamble lets the channel estimate be interpolated over the
frame, a ``TrackingPoint`` per link point switches either on; ``tracking_equalise`` states the definition in fp64,
``frame_profile_tracking`` and ``rx_profile_tracking_host`` mirror the call.

``rx_profile_coset_gpu`` (``wofdm_rx_profile_coset``) runs the Viterbi and the LDPC decoders of the coded link behind one receive
chain against RANDOM transmitted words -- the frame's information stream (``coset_info``, Philox stream 4) encoded on the GPU --
where the coded calls count against the all-zero word; ``coset_codewords`` gives the transmitted words, ``conv_encode_gpu`` and
``ldpc_encode_gpu`` are the encoders alone, ``frame_profile_coset`` and ``rx_profile_coset_host`` mirror the call.
"""
import collections

import numpy as np

RxProfile = collections.namedtuple("RxProfile", "bit_err sym_err err_power decisions")
RxProfile.__doc__ = """bit_err, sym_err (uint64), err_power (float64): [pairs, n_snr, n_ch, N]; decisions [N]: hard decisions a
bin took per cell = frames * (S - 1) on the loaded bins, 0 on the others."""

RxProfileSync = collections.namedtuple("RxProfileSync", "bit_err sym_err err_power bit_err_sym sym_err_sym err_power_sym decisions")
RxProfileSync.__doc__ = """bit_err, sym_err (uint64), err_power (float64): [points, pairs, n_snr, n_ch, N] as ``RxProfile``'s per
point; bit_err_sym, sym_err_sym (uint64), err_power_sym (float64): [points, pairs, n_snr, n_ch, S - 1], the same three sums
over the loaded bins per data symbol s = 1 ... S - 1; decisions [N] as ``RxProfile``'s (per point)."""

SyncPoint = collections.namedtuple("SyncPoint", "timing cfo cfo_tracked", defaults=(0.0, 1))
SyncPoint.__doc__ = """One receiver offset of ``wofdm_rx_profile_sync``: timing (theta, samples: the receive windows begin theta
samples late (> 0) or early (< 0), |theta| < B), cfo (epsilon, in subcarrier spacings, |epsilon| <= 4, used as stored in
single precision), cfo_tracked (0: free-running oscillator, every sample rotated by e^{2 pi i epsilon a / N} at its on-air
index a; 1: the common phase of every symbol removed, e^{2 pi i epsilon m / N} at index m under the window)."""

NEAR_TOL = 1e-4


# ---- the slicer and the helpers on the counters ----

def slice_labels(bits_per_sc, z):
    """``qamdemod`` hard decision (main_BER_calculation.m:269-270): MATLAB Gray label of the nearest point of the unit-power
    constellation, the first bit of the subcarrier on top (``timefreq.qam_table`` is its inverse)."""
    k = int(bits_per_sc)
    half = k // 2
    m = 1 << half
    a = np.sqrt(2.0 * (m * m - 1) / 3.0)
    z = np.asarray(z, dtype=np.complex128)
    ii = np.clip(np.floor((z.real * a + (m - 1)) * 0.5 + 0.5), 0, m - 1).astype(np.int64)
    qi = np.clip(np.floor(((m - 1) - z.imag * a) * 0.5 + 0.5), 0, m - 1).astype(np.int64)
    return ((ii ^ (ii >> 1)) << half) | (qi ^ (qi >> 1))


def threshold_distance(bits_per_sc, z):
    """Distance of the nearer component of z to the nearest slicer threshold that matters (the outer regions have none
    beyond the last threshold), in constellation units."""
    k = int(bits_per_sc)
    m = 1 << (k // 2)
    a = np.sqrt(2.0 * (m * m - 1) / 3.0)
    z = np.asarray(z, dtype=np.complex128)

    def comp(v):
        t = (v * a + (m - 1)) * 0.5 + 0.5           # thresholds at the integers 1 .. m - 1
        near = np.clip(np.round(t), 1, m - 1)
        return np.abs(t - near) * 2.0 / a
    return np.minimum(comp(z.real), comp(-z.imag))


def near_decisions(bits_per_sc, xhat, y0, tol=NEAR_TOL):
    """[S-1, N] bool: decisions that single-precision rounding may tip -- a component of the fp64 ``xhat`` [S-1, N] lies
    within tol * max(1, |xhat|) * max_n |y0| / |y0[n]| of a slicer threshold (y0 [N]: the received pilot; 0 = unloaded).  y0
    [S-1, N]: the estimate every symbol is equalised with (a tracking receiver's), the maximum taken per symbol; 0 = no decision."""
    xhat = np.asarray(xhat, dtype=np.complex128)
    a0 = np.atleast_2d(np.abs(np.asarray(y0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = tol * np.maximum(1.0, np.abs(xhat)) * (a0.max(axis=-1, keepdims=True) / a0)
    return (threshold_distance(bits_per_sc, xhat) <= bound) & (a0 > 0)


def ber_per_bin(prof, bits_per_sc):
    """Bit error rate per subcarrier [pairs, n_snr, n_ch, N]; NaN on unloaded bins."""
    d = _decisions_like(prof.decisions, prof.bit_err) * int(bits_per_sc)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, prof.bit_err / np.where(d > 0, d, 1.0), np.nan)


def evm_db(prof):
    """Error-vector magnitude per subcarrier in dB relative to the constellation's unit average power:
    10 log10(err_power / decisions); NaN on unloaded bins."""
    d = _decisions_like(prof.decisions, prof.err_power)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, 10.0 * np.log10(prof.err_power / np.where(d > 0, d, 1.0)), np.nan)


def _decisions_like(dec, arr):
    """The decisions as float64, broadcastable against ``arr`` [..., n]: [n] as they are; per point [points, n] (a tracking
    receiver's) with the axes between the point's and the last of ``arr`` [points, ..., n] as ones"""
    dec = np.asarray(dec).astype(np.float64)
    return dec if dec.ndim == 1 else dec.reshape((dec.shape[0],) + (1,) * (np.ndim(arr) - 2) + (dec.shape[1],))


# ---- fp64 host mirror ----

def frame_profile(st, grids, unit_noise, w_tx, w_rx, h, snr_db, bits_per_sc, active=None, mask=None,
                  noise_before_truncate=1):
    """fp64 host mirror of one frame of ``wofdm_rx_profile`` (main_BER_calculation.m:253-272,
    277-355).  grids [S, N]: the transmitted constellation points (zeros on unloaded bins);
    unit_noise [noise_len] complex; w_tx [P], w_rx [N + delta], h [taps].  Returns (bit_err [N], sym_err [N], err_power
    [N], xhat [S-1, N], y0 [N]); unloaded bins are 0 everywhere."""
    return _frame_steps(st, grids, unit_noise, w_tx, w_rx, h, snr_db, bits_per_sc, active, mask, noise_before_truncate)[:5]


def _frame_steps(st, grids, unit_noise, w_tx, w_rx, h, snr_db, bits_per_sc, active, mask, noise_before_truncate, beside=None):
    """The steps of ``frame_profile``; beside(S, B) -> [S B] complex or None: what another transmitter adds to the truncated
    received samples (after the noise, whose gain never sees it).  Returns frame_profile's five outputs and Y [S, N]."""
    from . import timefreq as T
    X = np.asarray(grids, dtype=np.complex128)
    n, delta, gam, k = st.n_fft, st.tail_rx, st.prefix_rm, int(bits_per_sc)
    S, B = X.shape[0], st.sym_len - st.tail_tx
    if X.shape != (S, n) or B != n + delta + gam:
        raise ValueError("grids must be [S, %d] and the structure consistent" % n)
    on = np.ones(n, dtype=bool) if active is None else np.asarray(active).reshape(-1) != 0
    tx = T.tx_waveform(st, X.T, np.asarray(w_tx, np.float64), st.tail_tx, mask, guard_band=None)
    conv = np.convolve(np.asarray(h, dtype=np.complex128).reshape(-1), tx)           # m:260
    noise = np.asarray(unit_noise, dtype=np.complex128).reshape(-1)
    nl = conv.size if noise_before_truncate else S * B
    if noise.size < nl:
        raise ValueError("unit_noise holds %d samples, %d needed" % (noise.size, nl))
    ps, pn = np.mean(np.abs(conv[:nl]) ** 2), np.mean(np.abs(noise[:nl]) ** 2)       # add_wgn, m:277-294
    g = np.sqrt(ps * 10.0 ** (-0.1 * float(snr_db)) / pn)
    r = conv[:S * B] + g * noise[:S * B]                                             # truncate, m:261-263
    other = None if beside is None else beside(S, B)
    r = (r if other is None else r + other).reshape(S, B)
    blocks = r[:, gam:gam + n + delta] * np.asarray(w_rx, np.float64)[None, :]       # wofdm_rx, m:297-355
    z = blocks[:, :n].copy()
    z[:, :delta] += blocks[:, n:]
    Y = np.fft.fft(np.roll(z, -(st.circ_shift + delta // 2), axis=1), axis=1)
    xhat = np.zeros((S - 1, n), dtype=np.complex128)
    xhat[:, on] = Y[1:, on] / (Y[0, on] / X[0, on])[None, :]                         # m:266-268
    d = np.where(on[None, :], slice_labels(k, X[1:]) ^ slice_labels(k, xhat), 0)
    bits = sum((d >> b) & 1 for b in range(k))
    err = np.where(on[None, :], np.abs(xhat - X[1:]) ** 2, 0.0)
    return (bits.sum(axis=0).astype(np.uint64), (d != 0).sum(axis=0).astype(np.uint64), err.sum(axis=0), xhat,
            np.where(on, Y[0], 0.0), Y)


def frame_profile_aci(st, grids, aci_grids, unit_noise, w_tx, w_rx, h, aci_h, delay, level_db, snr_db, bits_per_sc,
                      active=None, mask=None, noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame of ``wofdm_rx_profile_aci``: ``frame_profile`` (its own steps) with an adjacent-band
    neighbour beside the victim.  aci_grids [S + 1, N]: the neighbour's constellation points (zeros on the bins it leaves
    free), sent through the victim's Tx chain (w_tx, mask) as a waveform xi of tail_tx + (S + 1) B samples; its symbol u
    begins at victim time (u - 1) B + delay, 0 <= delay < B, so the victim's on-air sample t carries a xi[t + B - delay], a
    = 10^(level_db / 20); it passes aci_h [taps] (None: h) -- what it sent before t = 0 included --, and is added to the
    received samples after the noise: Ps, Pn and the noise gain are the victim's alone.  Returns what ``frame_profile``
    returns (with an all-zero aci_grids the same arrays); with_y=True: Y [S, N] as a sixth output."""
    Xi = np.asarray(aci_grids, dtype=np.complex128)
    S = np.asarray(grids).shape[0]
    B, d = st.sym_len - st.tail_tx, int(delay)
    if Xi.shape != (S + 1, st.n_fft):
        raise ValueError("aci_grids must be [S + 1, %d]" % st.n_fft)
    if not 0 <= d < B:
        raise ValueError("delay must lie in [0, %d)" % B)
    def beside(S_, B_):
        return _aci_on_air(st, Xi, w_tx, h if aci_h is None else aci_h, level_db, mask)[B_ - d:B_ - d + S_ * B_]
    out = _frame_steps(st, grids, unit_noise, w_tx, w_rx, h, snr_db, bits_per_sc, active, mask, noise_before_truncate, beside)
    return out if with_y else out[:5]


def _aci_on_air(st, Xi, w_tx, hi, level_db, mask):
    """The neighbour of ``frame_profile_aci`` as received: 10^(level_db / 20) conv(hi, xi), xi the waveform of its grids Xi [S +
    1, N] through the victim's Tx chain; the victim's on-air sample t carries element t + B - delay of it."""
    from . import timefreq as T
    xi = T.tx_waveform(st, np.asarray(Xi).T, np.asarray(w_tx, np.float64), st.tail_tx, mask, guard_band=None)
    return 10.0 ** (0.05 * float(level_db)) * np.convolve(np.asarray(hi, dtype=np.complex128).reshape(-1), xi)


# ---- the random streams of csrc/philox.h on the host ----

def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words"""
    lo = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & lo for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & lo, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & lo, (k1 + np.uint64(0xBB67AE85)) & lo
    return np.stack([c0, c1, c2, c3], axis=-1)


def _stream(seed, stream, cell, frame, n_blocks):
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    return _philox(np.arange(n_blocks, dtype=np.uint64), frame & 0xFFFFFFFF, frame >> 32,
                   (stream << 28) | (int(cell) & 0x0FFFFFFF), seed & 0xFFFFFFFF, seed >> 32)


STREAM_BITS, STREAM_NOISE, STREAM_ACI, STREAM_PN = 0, 1, 2, 3   # csrc/philox.h


def gen_labels(n_fft, bits_per_sc, syms, seed, cell, frame, stream=0):
    """[S, N] uint8 labels of stream 0 of (seed, cell, frame): csrc/philox.h, what a plan draws.  stream=2
    (``STREAM_ACI``): the labels of the neighbour of ``wofdm_rx_profile_aci``, the same layout on its own stream."""
    k = int(bits_per_sc)
    ks = 8 if k == 6 else k
    bps = n_fft * ks // 128
    w = _stream(seed, int(stream), cell, frame, syms * bps).reshape(syms, bps * 4)
    bit = np.arange(n_fft, dtype=np.int64) * ks
    return ((w[:, bit >> 5] >> (bit & 31).astype(np.uint64)[None, :]) & np.uint64((1 << k) - 1)).astype(np.uint8)


def gen_noise(noise_len, seed, cell, frame):
    """[noise_len] complex unit normals of stream 1 of (seed, cell, frame): the uniforms in single precision as the kernels
    form them, Box-Muller in double."""
    w = _stream(seed, 1, cell, frame, (noise_len + 1) // 2).reshape(-1, 2)[:noise_len]
    u1 = (w[:, 0].astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)
    u2 = (w[:, 1] >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * u2)


def gen_noise_at(idx, seed, cell, frame):
    """Complex unit normals of stream 1 of (seed, cell, frame) at the sample indices ``idx`` (any integers, any shape): sample a
    is that of counter word a mod 2^32 -- block (a mod 2^32) >> 1, word pair a & 1 --, so on [0, noise_len) this is
    ``gen_noise`` and a negative index lands on words no frame uses."""
    a = np.asarray(idx, dtype=np.int64) & np.int64(0xFFFFFFFF)
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    w = _philox((a >> 1).astype(np.uint64), frame & 0xFFFFFFFF, frame >> 32, (1 << 28) | (int(cell) & 0x0FFFFFFF),
                seed & 0xFFFFFFFF, seed >> 32)
    odd = (a & 1) != 0
    w0, w1 = np.where(odd, w[..., 2], w[..., 0]), np.where(odd, w[..., 3], w[..., 1])
    u1 = (w0.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)
    u2 = (w1 >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * u2)


def _noise_len(st, syms, n_taps, noise_before_truncate):
    B = st.sym_len - st.tail_tx
    return st.tail_tx + syms * B + n_taps - 1 if noise_before_truncate else syms * B


def _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask):
    from . import _lib
    w_tx = _lib.f32(np.atleast_2d(w_tx_pairs))
    w_rx = _lib.f32(np.atleast_2d(w_rx_pairs))
    if w_tx.shape[1] != st.sym_len or w_rx.shape != (w_tx.shape[0], st.n_fft + st.tail_rx):
        raise ValueError("windows must be [pairs, %d] and [pairs, %d]" % (st.sym_len, st.n_fft + st.tail_rx))
    hc = np.ascontiguousarray(np.atleast_2d(h), dtype=np.complex64)
    snr = _lib.f32(np.atleast_1d(snr_db))
    act = None if active is None else np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, dtype=np.uint8)
    if act is not None and act.shape != (st.n_fft,):
        raise ValueError("active must hold %d flags" % st.n_fft)
    m = None if mask is None else _lib.f32(np.asarray(mask).reshape(-1), (2 * st.sym_len - 1,))
    return w_tx, w_rx, hc, snr, act, m


def _decisions(st, syms, frames, act):
    on = np.ones(st.n_fft, dtype=bool) if act is None else act != 0
    return np.where(on, int(frames) * (int(syms) - 1), 0).astype(np.uint64)


# ---- the host sweep and the GPU call every arm goes through ----

#: what ``_host_sweep`` hands an arm: the prepared arguments (single precision, as the GPU receives them), k, S, the noise
#: samples a frame needs (``_noise_len``) and the seed
_Sweep = collections.namedtuple("_Sweep", "st k S w_tx w_rx hc snr act m nbt noise_len seed")


def _host_sweep(result, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, active, mask,
                noise_before_truncate, with_near, n_scales=None):
    """The host route of every arm: the cells (pair, SNR point, channel) of the sweep and their frames [frame_offset,
    frame_offset + frames), the labels of stream 0 drawn per frame, the sums kept per field of ``result`` (a namedtuple type
    whose last field is ``decisions``: per bin [N], ``*_sym`` per data symbol [S - 1], ``pa_power`` [2], ``bit_penalty*`` with
    the ``n_scales`` scales before that axis; the counters uint64, the powers and penalties float64, added up frame by frame).  arm(q: ``_Sweep``) does the arm's own argument preparation and returns
    (lead, frame): lead = () or (n_points,), the leading axis of every sum, and frame(p, s, c, cell, fr, grid) -> per point
    one tuple (bit_err, sym_err, err_power, xhat, y0, then the further fields of ``result`` in its order; anything behind is
    ignored), for which the arm draws what the frame needs beyond the labels.  Returns ``result``, and with_near=True also the
    number of ``near_decisions`` per point and cell."""
    from . import timefreq as T
    w_tx, w_rx, hc, snr, act, m = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pairs, n_snr, n_ch, n = w_tx.shape[0], snr.size, hc.shape[0], st.n_fft
    k, S = int(bits_per_sc), int(syms)
    lead, frame = arm(_Sweep(st, k, S, w_tx, w_rx, hc, snr, act, m, noise_before_truncate,
                             _noise_len(st, S, hc.shape[1], noise_before_truncate), seed))
    tab = T.qam_table(k)
    on = np.ones(n, dtype=bool) if act is None else act != 0
    shape = lead + (pairs, n_snr, n_ch)
    sums = [np.zeros(shape + ((int(n_scales),) if f.startswith("bit_penalty") else ()) +
                     ((2,) if f == "pa_power" else (S - 1,) if f.endswith("_sym") else (n,)),
                     dtype=np.float64 if "power" in f or "penalty" in f else np.uint64) for f in result._fields[:-1]]
    near = np.zeros(shape, dtype=np.int64)
    for cell in range(pairs * n_snr * n_ch):
        p, s, c = cell // (n_snr * n_ch), (cell // n_ch) % n_snr, cell % n_ch
        for f in range(int(frames)):
            fr = int(frame_offset) + f
            grid = tab[gen_labels(n, k, S, seed, cell, fr)] * on[None, :]
            for i, o in enumerate(frame(p, s, c, cell, fr, grid)):
                at = (i, p, s, c) if lead else (p, s, c)
                for a, v in zip(sums, o[:3] + o[5:]):
                    a[at] += v
                if with_near:
                    near[at] += int(near_decisions(k, o[3], o[4]).sum())
    prof = result(*sums, _decisions(st, S, frames, act))
    return (prof, near) if with_near else prof


def _plain_arm(q):
    """``rx_profile_host``'s arm: the frame's unit noise, ``frame_profile``"""
    def frame(p, s, c, cell, fr, grid):
        return [frame_profile(q.st, grid, gen_noise(q.noise_len, q.seed, cell, fr), q.w_tx[p], q.w_rx[p], q.hc[c], q.snr[s],
                              q.k, q.act, q.m, q.nbt)]
    return (), frame


def rx_profile_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, active=None,
                    mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_gpu``: the same frames from the same Philox streams, each through
    ``frame_profile`` (single-precision inputs as the GPU receives them, fp64 arithmetic).  with_near=True: also the
    number of ``near_decisions`` per cell [pairs, n_snr, n_ch]."""
    return _host_sweep(RxProfile, _plain_arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                       active, mask, noise_before_truncate, with_near)


def _noise_lookup(noise, lo=0):
    """noise_at(idx) of ``_sync_front`` and the point functions on a frame's samples [lo, lo + len(noise))"""
    def noise_at(idx):
        return noise[np.asarray(idx, dtype=np.int64) - lo]
    return noise_at


def _unit_noise_lookup(st, grids, unit_noise, n_taps, noise_before_truncate):
    """The same on the ``unit_noise`` argument of a frame mirror, which must hold the frame's ``_noise_len`` samples"""
    noise = np.asarray(unit_noise, dtype=np.complex128).reshape(-1)
    nl = _noise_len(st, np.asarray(grids).shape[0], n_taps, noise_before_truncate)
    if noise.size < nl:
        raise ValueError("unit_noise holds %d samples, %d needed" % (noise.size, nl))
    return _noise_lookup(noise)


def _chunk_frames(st, syms, masked, per_point=0, n_points=0, per_frame_extra=0, neighbour=False, extra_bytes=0):
    """Frames one chunk holds: the byte budget of include/wofdm.h (``rx_job_bytes`` of wofdm_abi.hip) over the bytes of a frame
    -- 8 per element: the symbol grid [S, N], the waveform [T], masked the filtered symbols [S, 2P - 1]; with a neighbour
    its grid [S + 1, N], waveform [T + B] and filtered symbols; ``per_frame_extra`` elements of the arm's own; ``per_point``
    elements (the partial sums, a waveform) for each of ``n_points``; ``extra_bytes`` bytes that are no 8-byte elements --, at
    least 1, at most 65535."""
    from . import _lib
    P, B = st.sym_len, st.sym_len - st.tail_tx
    T = st.tail_tx + syms * B
    words = syms * st.n_fft + T + (syms * (2 * P - 1) if masked else 0)
    if neighbour:
        words += (syms + 1) * st.n_fft + T + B + ((syms + 1) * (2 * P - 1) if masked else 0)
    per_frame = 8 * (words + per_frame_extra + int(n_points) * per_point) + int(extra_bytes)
    return min(65535, max(1, _lib.RX_PROFILE_CHUNK_BYTES // per_frame))


def _gpu_call(entry, result, st, bits_per_sc, syms, prepared, seed, frame_offset, frames, noise_before_truncate, device, out,
              lead=(), after_h=(), after_mask=(), n_ch=None, n_scales=None, behind=()):
    """One call of the library's receive-profile entry point ``entry``: prepared = ``_prepare``'s six (the fifth argument of
    the entry point is prepared[2], of any rank, taps last; n_ch: its channels where they are not its first axis); after_h,
    after_mask: the arm's own ctypes arguments, behind h and behind the mask; lead = () or (n_points,).  The outputs are
    those ``result`` has fields for -- the {bit, symbol} counters and the power per bin; with ``*_sym`` fields the same per
    data symbol; with ``pa_power`` the power sums; with ``bit_penalty`` the penalties of the ``n_scales`` scales per bin and per
    data symbol --, each behind the leading axes lead + (pairs, n_snr, n_ch).  Returns
    ``result``, added to ``out`` (an earlier result of the same shape) where given."""
    import ctypes as C
    from . import _lib
    from .simulation import make_cfg
    w_tx, w_rx, hc, snr, act, m = prepared
    pairs, n_snr, n_ch = w_tx.shape[0], snr.size, hc.shape[0] if n_ch is None else n_ch
    cfg = make_cfg(st, int(bits_per_sc), int(syms), hc.shape[-1], n_ch, n_snr, pairs, bool(noise_before_truncate),
                   seed=int(seed), frames_per_cell=int(frames), frame_offset=int(frame_offset))
    shape = tuple(lead) + (pairs, n_snr, n_ch)
    tails = [(st.n_fft,)] + [(int(syms) - 1,)] * ("bit_err_sym" in result._fields)
    outs = []
    for tail in tails:
        outs += [np.zeros(shape + tail + (2,), dtype=np.uint64), np.zeros(shape + tail, dtype=np.float64)]
    if "pa_power" in result._fields:
        outs.append(np.zeros(shape + (2,), dtype=np.float64))
    if "bit_penalty" in result._fields:
        outs += [np.zeros(shape + (int(n_scales),) + tail, dtype=np.float64) for tail in tails]
    hf = _lib.c64_as_f32(hc)
    _lib.check(getattr(_lib.load(), entry)(
        C.byref(cfg), int(device), w_tx.ctypes.data, w_rx.ctypes.data, hf.ctypes.data, *after_h, snr.ctypes.data,
        None if act is None else act.ctypes.data, None if m is None else m.ctypes.data, *after_mask,
        *(a.ctypes.data for a in outs), *behind))                      # (behind: the entry point's arguments after the outputs)
    fields = []
    for a in outs:
        fields += [np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1])] if a.dtype == np.uint64 else [a]
    prof = result(*fields, _decisions(st, syms, frames, act))
    if out is not None:
        if out.bit_err.shape != prof.bit_err.shape:
            raise ValueError("out has another shape")
        prof = result(*(a + b for a, b in zip(out, prof)))
    return prof


# ---- GPU ----

def rx_profile_chunk_frames(st, syms, masked):
    """Frames one chunk of ``wofdm_rx_profile`` holds (include/wofdm.h: WOFDM_RX_PROFILE_CHUNK_BYTES over the bytes of a
    frame's symbol grid, waveform, -- masked -- filtered symbols and per-bin partial sums; at most 65535)."""
    return _chunk_frames(st, syms, masked, per_point=st.n_fft, n_points=1)


def rx_profile_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, active=None,
                   mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile``: per-subcarrier bit errors, symbol errors and error power of the frames [frame_offset,
    frame_offset + frames) of every cell of the sweep w_tx_pairs [pairs, P] x w_rx_pairs [pairs, N + delta] x snr_db
    [n_snr] x h [n_ch, taps] -- drawn as a ``Plan`` of the same cfg and seed draws them, with the allocation ``active`` [N]
    and the Tx mask ``mask`` [2P-1].  Returns ``RxProfile``; ``out`` (an earlier result of the same shape) is accumulated
    into, its ``decisions`` added up.  No CPU fallback."""
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    return _gpu_call("wofdm_rx_profile", RxProfile, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                     noise_before_truncate, device, out)


# ---- beside an adjacent-band neighbour (wofdm_rx_profile_aci) ----

def _prepare_aci(st, hc, aci_active, aci_h, aci_delay, aci_level_db):
    iact = np.ascontiguousarray(np.asarray(aci_active).reshape(-1) != 0, dtype=np.uint8)
    if iact.shape != (st.n_fft,):
        raise ValueError("aci_active must hold %d flags" % st.n_fft)
    hi = None if aci_h is None else np.ascontiguousarray(np.atleast_2d(aci_h), dtype=np.complex64)
    if hi is not None and hi.shape != hc.shape:
        raise ValueError("aci_h must have the shape of h, %s" % (hc.shape,))
    return iact, hi, int(aci_delay), float(np.float32(aci_level_db))


def rx_profile_aci_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, aci_active,
                        aci_delay, aci_level_db=0.0, aci_h=None, active=None, mask=None, noise_before_truncate=1,
                        with_near=False):
    """The host route of ``rx_profile_aci_gpu``: the frames of ``rx_profile_host`` with the neighbour's S + 1 symbols of
    stream 2 on ``aci_active`` beside each, through ``frame_profile_aci``.  An ``aci_active`` without a loaded bin is
    ``rx_profile_host``.  with_near=True: also the number of ``near_decisions`` per cell [pairs, n_snr, n_ch]."""
    from . import timefreq as T

    def arm(q):
        iact, hi, d, lvl = _prepare_aci(st, q.hc, aci_active, aci_h, aci_delay, aci_level_db)
        if not iact.any():
            return _plain_arm(q)
        tab = T.qam_table(q.k)

        def frame(p, s, c, cell, fr, grid):
            igrid = tab[gen_labels(st.n_fft, q.k, q.S + 1, seed, cell, fr, STREAM_ACI)] * (iact != 0)[None, :]
            return [frame_profile_aci(st, grid, igrid, gen_noise(q.noise_len, seed, cell, fr), q.w_tx[p], q.w_rx[p], q.hc[c],
                                      None if hi is None else hi[c], d, lvl, q.snr[s], q.k, q.act, q.m, q.nbt)]
        return (), frame
    return _host_sweep(RxProfile, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                       active, mask, noise_before_truncate, with_near)


def rx_profile_aci_chunk_frames(st, syms, masked):
    """Frames one chunk of ``wofdm_rx_profile_aci`` holds with a neighbour (include/wofdm.h: both symbol grids, S and S + 1
    symbols, both waveforms, T and T + B samples, -- masked -- both sets of filtered symbols, the per-bin partials; at most
    65535).  Without one (an empty ``aci_active``) the call chunks as ``rx_profile_chunk_frames``."""
    return _chunk_frames(st, syms, masked, per_point=st.n_fft, n_points=1, neighbour=True)


def rx_profile_aci_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, aci_active,
                       aci_delay, aci_level_db=0.0, aci_h=None, active=None, mask=None, noise_before_truncate=1, device=0,
                       out=None):
    """``wofdm_rx_profile_aci``: ``rx_profile_gpu`` of the same arguments with an asynchronous adjacent-band neighbour on the
    air -- the victim's numerology, Tx window and mask on the bins ``aci_active`` [N], S + 1 symbols of label stream 2, its
    symbol u beginning at victim time (u - 1) B + ``aci_delay`` (0 <= aci_delay < B), amplitude 10^(aci_level_db / 20),
    through ``aci_h`` [n_ch, taps] (None: h).  The SNR stays the victim's.  Returns ``RxProfile`` on the victim's loaded
    bins; ``out`` is accumulated into.  No CPU fallback."""
    from . import _lib
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    iact, hi, d, lvl = _prepare_aci(st, prepared[2], aci_active, aci_h, aci_delay, aci_level_db)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    return _gpu_call("wofdm_rx_profile_aci", RxProfile, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                     noise_before_truncate, device, out,
                     after_mask=(iact.ctypes.data, None if hif is None else hif.ctypes.data, d, lvl))


def rx_profile_kernel_ms():
    """Milliseconds the kernels of this thread's last ``rx_profile_gpu``, ``rx_profile_aci_gpu``, ``rx_profile_sync_gpu``,
    ``rx_profile_doppler_gpu``, ``rx_profile_pa_gpu``, ``rx_profile_pn_gpu`` or ``rx_profile_link_gpu`` call took (``wofdm_rx_profile_kernel_ms``)."""
    import ctypes as C
    from . import _lib
    ms = C.c_float()
    _lib.check(_lib.load().wofdm_rx_profile_kernel_ms(C.byref(ms)))
    return float(ms.value)


# ---- under receiver timing and carrier-frequency offset (wofdm_rx_profile_sync) ----

def _sync_front(st, grids, noise_at, w_tx, h, snr_db, active, mask, noise_before_truncate, channel=None):
    """What the points of a frame share: X [S, N], conv(h, x) [T + taps - 1], the noise gain g (``frame_profile``'s: the
    offsets never touch it) and the loaded bins.  channel(x) -> what is received of the waveform x in conv(h, x)'s place (a
    channel that moves within the frame: ``frame_profile_doppler``); h is not read then."""
    from . import timefreq as T
    X = np.asarray(grids, dtype=np.complex128)
    n = st.n_fft
    S, B = X.shape[0], st.sym_len - st.tail_tx
    if X.shape != (S, n) or B != n + st.tail_rx + st.prefix_rm:
        raise ValueError("grids must be [S, %d] and the structure consistent" % n)
    on = np.ones(n, dtype=bool) if active is None else np.asarray(active).reshape(-1) != 0
    tx = T.tx_waveform(st, X.T, np.asarray(w_tx, np.float64), st.tail_tx, mask, guard_band=None)
    conv = np.convolve(np.asarray(h, dtype=np.complex128).reshape(-1), tx) if channel is None else channel(tx)
    nl = conv.size if noise_before_truncate else S * B
    noise = np.asarray(noise_at(np.arange(nl, dtype=np.int64)), dtype=np.complex128)
    ps, pn = np.mean(np.abs(conv[:nl]) ** 2), np.mean(np.abs(noise) ** 2)
    return X, conv, np.sqrt(ps * 10.0 ** (-0.1 * float(snr_db)) / pn), on


def _sync_point(st, front, noise_at, w_rx, point, bits_per_sc, beside=None, phase=None):
    """One point on a frame's shared part: ``frame_profile_sync``'s outputs and Y [S, N].  ``frame_profile_link``'s further
    stages, on the on-air indices a [S, N + delta] of the samples under the windows: beside(a) -> what another transmitter adds
    to them (after the noise); phase(a) -> a second rotation behind the carrier offset's."""
    X, conv, g, on = front
    n, delta, gam, k = st.n_fft, st.tail_rx, st.prefix_rm, int(bits_per_sc)
    S, B = X.shape[0], st.sym_len - st.tail_tx
    theta, eps = int(point.timing), float(np.float32(point.cfo))
    if abs(theta) >= B or not abs(eps) <= 4.0 or point.cfo_tracked not in (0, 1):
        raise ValueError("a point needs |timing| < %d, |cfo| <= 4 and cfo_tracked in (0, 1)" % B)
    m = np.arange(n + delta, dtype=np.int64)
    a = (np.arange(S, dtype=np.int64) * B + gam + theta)[:, None] + m[None, :]          # on-air index of every sample used
    inside = (a >= 0) & (a < conv.size)
    r = np.where(inside, conv[np.clip(a, 0, conv.size - 1)], 0.0) + g * np.asarray(noise_at(a), dtype=np.complex128)
    if beside is not None:
        r = r + beside(a)
    turns = eps * (m[None, :] if point.cfo_tracked else a).astype(np.float64) / n      # (exact: 24 bits times an integer)
    r = r * np.exp(2j * np.pi * (turns - np.round(turns)))
    return _point_outputs(st, X, on, r if phase is None else r * phase(a), w_rx, k)


def _point_outputs(st, X, on, r, w_rx, k):
    """The receiver behind the oscillator, for the arms with a point loop: r [S, N + delta], the received samples under the
    symbols' windows, rotated -> ``_sync_point``'s outputs"""
    n, delta, S = st.n_fft, st.tail_rx, X.shape[0]
    blocks = r * np.asarray(w_rx, np.float64)[None, :]
    z = blocks[:, :n].copy()
    z[:, :delta] += blocks[:, n:]
    Y = np.fft.fft(np.roll(z, -(st.circ_shift + delta // 2), axis=1), axis=1)
    xhat = np.zeros((S - 1, n), dtype=np.complex128)
    xhat[:, on] = Y[1:, on] / (Y[0, on] / X[0, on])[None, :]
    d = np.where(on[None, :], slice_labels(k, X[1:]) ^ slice_labels(k, xhat), 0)
    bits = sum((d >> b) & 1 for b in range(k))
    err = np.where(on[None, :], np.abs(xhat - X[1:]) ** 2, 0.0)
    return (bits.sum(axis=0).astype(np.uint64), (d != 0).sum(axis=0).astype(np.uint64), err.sum(axis=0), xhat,
            np.where(on, Y[0], 0.0), bits.sum(axis=1).astype(np.uint64), (d != 0).sum(axis=1).astype(np.uint64),
            err.sum(axis=1), Y)


def frame_profile_sync(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, active=None, mask=None,
                       noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_sync``: ``frame_profile`` with the receive windows
    moved by ``point.timing`` samples and the oscillator off by ``point.cfo`` subcarrier spacings.  noise_at(idx) -> the
    complex unit normals at the integer sample indices idx (``gen_noise_at`` of the frame): the received signal is r[a] =
    conv(h, x)[a] + g n[a] for every integer a, conv zero outside [0, T + taps - 1), g from Ps and Pn over [0, noise_len) as
    in ``frame_profile``; sample m of symbol s sits at a = s B + prefix_rm + timing + m and is multiplied by e^{2 pi i cfo a /
    N} (free-running) or e^{2 pi i cfo m / N} (tracked) before the Rx window; the pilot sees the same offsets.  Returns
    (bit_err [N], sym_err [N], err_power [N], xhat [S-1, N], y0 [N], bit_err_sym [S-1], sym_err_sym [S-1], err_power_sym
    [S-1]) -- the first five are ``frame_profile``'s, exactly, at timing = 0, cfo = 0 --; with_y=True: Y [S, N] as a ninth."""
    front = _sync_front(st, grids, noise_at, w_tx, h, snr_db, active, mask, noise_before_truncate)
    out = _sync_point(st, front, noise_at, w_rx, point, bits_per_sc)
    return out if with_y else out[:8]


def _prepare_sync(points):
    pts = [SyncPoint(*q) for q in points]
    pts = [SyncPoint(int(q.timing), float(np.float32(q.cfo)), int(q.cfo_tracked)) for q in pts]
    if not pts:
        raise ValueError("at least one point is needed")
    return pts


def rx_profile_sync_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points,
                         active=None, mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_sync_gpu``: the frames of ``rx_profile_host`` from the same Philox streams, each through
    ``frame_profile_sync`` for every point of ``points`` (``SyncPoint`` or (timing, cfo, cfo_tracked) tuples); the Tx chain,
    the channel and the noise gain of a frame are shared by its points.  Returns ``RxProfileSync``; with_near=True: also the
    number of ``near_decisions`` per point and cell [points, pairs, n_snr, n_ch]."""
    def arm(q):
        pts = _prepare_sync(points)
        # the sample indices a frame's points read, as one range
        lo = min(0, st.prefix_rm + min(pt.timing for pt in pts))
        hi = max(q.noise_len, (q.S - 1) * (st.sym_len - st.tail_tx) + st.prefix_rm + max(pt.timing for pt in pts) + st.n_fft
                 + st.tail_rx)

        def frame(p, s, c, cell, fr, grid):
            noise_at = _noise_lookup(gen_noise_at(np.arange(lo, hi, dtype=np.int64), seed, cell, fr), lo)
            front = _sync_front(st, grid, noise_at, q.w_tx[p], q.hc[c], q.snr[s], q.act, q.m, q.nbt)
            return (_sync_point(st, front, noise_at, q.w_rx[p], pt, q.k)[:8] for pt in pts)
        return (len(pts),), frame
    return _host_sweep(RxProfileSync, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                       active, mask, noise_before_truncate, with_near)


def rx_profile_sync_chunk_frames(st, syms, masked, n_points):
    """Frames one chunk of ``wofdm_rx_profile_sync`` holds (include/wofdm.h: the symbol grid, the waveform and -- masked -- the
    filtered symbols of a frame, and per point its per-bin and per-symbol partials; at most 65535)."""
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms, n_points=n_points)


def rx_profile_sync_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points,
                        active=None, mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_sync``: ``rx_profile_gpu`` of the same arguments for every receiver offset of ``points``
    (``SyncPoint`` or (timing, cfo, cfo_tracked) tuples, at most ``_lib.SYNC_MAX_POINTS``) in ONE call -- the Tx chain and the
    power pass run once per frame --, per subcarrier and per data symbol.  Returns ``RxProfileSync``; ``out`` (an earlier
    result of the same shape) is accumulated into.  No CPU fallback."""
    from . import _lib
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts = _prepare_sync(points)
    cpts = (_lib.SyncPoint * len(pts))(*[_lib.SyncPoint(q.timing, q.cfo, q.cfo_tracked, 0) for q in pts])
    return _gpu_call("wofdm_rx_profile_sync", RxProfileSync, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                     noise_before_truncate, device, out, lead=(len(pts),), after_mask=(len(pts), cpts))


# ---- over a channel that moves within the frame (wofdm_rx_profile_doppler) ----

def tv_conv(track, knot_step, x):
    """The time-varying convolution of ``wofdm_rx_profile_doppler`` in double precision.  track [n_knots, taps]: knot q is the
    tap vector at on-air index q * knot_step; for the output index a, 0 <= a < len(x) + taps - 1, with q = min(a // knot_step,
    n_knots - 2) and f = (a - q * knot_step) / knot_step the taps are h_l[a] = K[q][l] + f (K[q+1][l] - K[q][l]) -- taken at the
    OUTPUT sample's time -- and the result is sum_l h_l[a] x[a - l].  It is formed as c_q[a] + f (c_{q+1}[a] - c_q[a]) from the
    knots' own convolutions c_q = np.convolve(K[q], x), the same sum by linearity: so a track of equal knots gives
    np.convolve(K[0], x), exactly.  The knots must reach the last output: (n_knots - 1) knot_step >= len(x) + taps - 2."""
    K = np.asarray(track, dtype=np.complex128)
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    ks = int(knot_step)
    if K.ndim != 2 or K.shape[0] < 2 or ks < 1:
        raise ValueError("track must be [n_knots >= 2, taps] and knot_step >= 1")
    a = np.arange(x.size + K.shape[1] - 1, dtype=np.int64)
    if (K.shape[0] - 1) * ks < a[-1]:
        raise ValueError("the knots end at sample %d, the convolution at %d" % ((K.shape[0] - 1) * ks, a[-1]))
    q = np.minimum(a // ks, K.shape[0] - 2)
    f = (a - q * ks).astype(np.float64) / ks
    c = np.zeros((K.shape[0], a.size), dtype=np.complex128)
    for i in np.union1d(q, q + 1):
        c[i] = np.convolve(K[i], x)
    return c[q, a] + f * (c[q + 1, a] - c[q, a])


def frame_profile_doppler(st, grids, unit_noise, w_tx, w_rx, track, knot_step, snr_db, bits_per_sc, active=None, mask=None,
                          noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame and one track of ``wofdm_rx_profile_doppler``: ``frame_profile`` with ``tv_conv(track,
    knot_step, x)`` in the place of conv(h, x) -- Ps, the noise gain and every received sample are those of the moving channel;
    the receiver, its pilot estimate from symbol 0 included, is unchanged.  unit_noise [noise_len] as ``frame_profile``'s.
    Returns what ``frame_profile_sync`` returns: (bit_err [N], sym_err [N], err_power [N], xhat [S-1, N], y0 [N], bit_err_sym
    [S-1], sym_err_sym [S-1], err_power_sym [S-1]) -- the first five are ``frame_profile``'s, exactly, on a track whose knots
    all equal h --; with_y=True: Y [S, N] as a ninth."""
    noise_at = _unit_noise_lookup(st, grids, unit_noise, np.asarray(track).shape[-1], noise_before_truncate)
    front = _sync_front(st, grids, noise_at, w_tx, None, snr_db, active, mask, noise_before_truncate,
                        channel=lambda x: tv_conv(track, knot_step, x))
    out = _sync_point(st, front, noise_at, w_rx, SyncPoint(0, 0.0, 1), bits_per_sc)
    return out if with_y else out[:8]


def _prepare_tracks(tracks):
    """[n_tracks, n_ch, n_knots, taps] complex64, as the GPU receives them"""
    tr = np.ascontiguousarray(tracks, dtype=np.complex64)
    if tr.ndim != 4 or tr.shape[0] < 1 or tr.shape[2] < 2:
        raise ValueError("tracks must be [n_tracks >= 1, n_ch, n_knots >= 2, taps]")
    return tr


def rx_profile_doppler_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, tracks, knot_step, snr_db, seed, frame_offset,
                            frames, active=None, mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_doppler_gpu``: the frames of ``rx_profile_host`` from the same Philox streams, each
    through ``frame_profile_doppler`` for every track of ``tracks`` [n_tracks, n_ch, n_knots, taps] (the cell's channel picks
    the track's row); the labels, the Tx waveform and the noise of a frame are shared by its tracks.  Returns
    ``RxProfileSync`` with a leading track axis; with_near=True: also the number of ``near_decisions`` per track and cell
    [n_tracks, pairs, n_snr, n_ch]."""
    tr = _prepare_tracks(tracks)

    def arm(q):
        def frame(p, s, c, cell, fr, grid):
            noise = gen_noise(q.noise_len, seed, cell, fr)
            return (frame_profile_doppler(st, grid, noise, q.w_tx[p], q.w_rx[p], tr[i, c], knot_step, q.snr[s], q.k, q.act, q.m,
                                          q.nbt) for i in range(tr.shape[0]))
        return (tr.shape[0],), frame
    return _host_sweep(RxProfileSync, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, tr[0, :, 0], snr_db, seed, frame_offset,
                       frames, active, mask, noise_before_truncate, with_near)


def rx_profile_doppler_chunk_frames(st, syms, masked, n_tracks):
    """Frames one chunk of ``wofdm_rx_profile_doppler`` holds (include/wofdm.h): ``rx_profile_sync_chunk_frames`` with the
    tracks for its points."""
    return rx_profile_sync_chunk_frames(st, syms, masked, n_tracks)


def rx_profile_doppler_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, tracks, knot_step, snr_db, seed, frame_offset,
                           frames, active=None, mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_doppler``: ``rx_profile_gpu`` of the same arguments over channels that move within the frame, for
    every track of ``tracks`` [n_tracks, n_ch, n_knots, taps] (at most ``_lib.DOPPLER_MAX_TRACKS`` tracks of
    ``_lib.DOPPLER_MAX_KNOTS`` knots, knot q the taps at on-air index q * knot_step, linear in between: ``tv_conv``) in ONE
    call -- the Tx chain runs once per frame, every track sees the same labels and noise --, per subcarrier and per data
    symbol.  Returns the ``RxProfileSync`` tuple with a leading track axis; ``out`` (an earlier result of the same shape) is
    accumulated into.  No CPU fallback."""
    tr = _prepare_tracks(tracks)
    w_tx, w_rx, _, snr, act, m = _prepare(st, w_tx_pairs, w_rx_pairs, tr[0, :, 0], snr_db, active, mask)
    return _gpu_call("wofdm_rx_profile_doppler", RxProfileSync, st, bits_per_sc, syms, (w_tx, w_rx, tr, snr, act, m), seed,
                     frame_offset, frames, noise_before_truncate, device, out, lead=(tr.shape[0],),
                     after_h=(tr.shape[0], tr.shape[2], int(knot_step)), n_ch=tr.shape[1])


# ---- behind a nonlinear power amplifier (wofdm_rx_profile_pa) ----

PA_LINEAR, PA_RAPP, PA_CLIP = 0, 1, 2                      # include/wofdm.h

PaPoint = collections.namedtuple("PaPoint", "model ibo_db smooth", defaults=(2.0,))
PaPoint.__doc__ = """One amplifier of ``wofdm_rx_profile_pa`` / ``wofdm_tx_psd_batch_pa``: model (``PA_LINEAR``: y = x; ``PA_RAPP``:
AM/AM of a solid-state amplifier with smoothness ``smooth`` = p in [0.5, 16]; ``PA_CLIP``: the soft limiter, its p -> infinity
limit), ibo_db (input back-off in [-40, 60]: a_sat^2 = reference power * 10^(ibo_db / 10)); ibo_db and smooth are used as
stored in single precision."""

RxProfilePa = collections.namedtuple("RxProfilePa",
                                     "bit_err sym_err err_power bit_err_sym sym_err_sym err_power_sym pa_power decisions")
RxProfilePa.__doc__ = """``RxProfileSync``'s fields with the amplifier's points on the leading axis, and pa_power (float64)
[points, pairs, n_snr, n_ch, 2] = {sum |x|^2, sum |y|^2} over the T on-air samples of the cell's frames, before and behind the
amplifier."""


def _pa_point(point):
    q = PaPoint(*point)
    q = PaPoint(int(q.model), float(np.float32(q.ibo_db)), float(np.float32(q.smooth)))
    if q.model not in (PA_LINEAR, PA_RAPP, PA_CLIP) or not -40.0 <= q.ibo_db <= 60.0 or \
            (q.model == PA_RAPP and not 0.5 <= q.smooth <= 16.0):
        raise ValueError("a point needs a known model, ibo_db in [-40, 60] and, for the Rapp model, smooth in [0.5, 16]: %r" % (q,))
    return q


def pa_gain(model, rho, smooth=2.0):
    """The amplifier's gain g(rho) in double precision, rho = |x| / a_sat (any shape, >= 0): 1 for ``PA_LINEAR``; (1 +
    rho^(2p))^(-1/(2p)) for ``PA_RAPP`` with p = smooth, evaluated above rho = 1 as (1 / rho) (1 + rho^(-2p))^(-1/(2p)) so that no
    finite rho overflows; 1 up to rho = 1 and 1 / rho above for ``PA_CLIP``.  g = 1 at rho = 0."""
    rho = np.asarray(rho, dtype=np.float64)
    if model == PA_LINEAR:
        return np.ones_like(rho)
    lo, hi = np.minimum(rho, 1.0), np.maximum(rho, 1.0)               # each form on its own side only
    if model == PA_CLIP:
        return np.where(rho > 1.0, 1.0 / hi, 1.0)
    if model != PA_RAPP:
        raise ValueError("unknown amplifier model %r" % (model,))
    p2 = 2.0 * float(smooth)
    return np.where(rho > 1.0, (1.0 / hi) * (1.0 + hi ** -p2) ** (-1.0 / p2), (1.0 + lo ** p2) ** (-1.0 / p2))


def pa_saturation(point, ref_power):
    """a_sat of a point: sqrt(ref_power 10^(ibo_db / 10)) in double precision, stored in single (as the library stores it)"""
    q = _pa_point(point)
    return float(np.float32(np.sqrt(float(ref_power) * 10.0 ** (0.1 * q.ibo_db))))


def pa_apply(x, point, ref_power):
    """y = g(|x| / a_sat) x in double precision: the waveform x behind the amplifier ``point`` (``PaPoint`` or (model, ibo_db,
    smooth)) whose back-off counts from ``ref_power``; the phase is untouched.  A ``PA_LINEAR`` point returns x itself."""
    q = _pa_point(point)
    x = np.asarray(x, dtype=np.complex128)
    if q.model == PA_LINEAR:
        return x
    return pa_gain(q.model, np.abs(x) / pa_saturation(q, ref_power), q.smooth) * x


def frame_profile_pa(st, grids, unit_noise, w_tx, w_rx, h, point, ref_power, snr_db, bits_per_sc, active=None, mask=None,
                     noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_pa``: ``frame_profile`` with the finished on-air
    waveform x (window, mask, overlap-add, the last ramp-down included) passed through ``pa_apply(x, point, ref_power)`` before
    the channel -- Ps, the noise gain and every received sample are those of the amplified waveform; the receiver, its pilot
    estimate from symbol 0 included, is unchanged.  Returns what ``frame_profile_sync`` returns and the two power sums:
    (bit_err [N], sym_err [N], err_power [N], xhat [S-1, N], y0 [N], bit_err_sym [S-1], sym_err_sym [S-1], err_power_sym [S-1],
    pa_power [2] = {sum |x|^2, sum |y|^2}) -- the first five are ``frame_profile``'s, exactly, on a ``PA_LINEAR`` point --;
    with_y=True: Y [S, N] as a tenth."""
    hc = np.asarray(h, dtype=np.complex128).reshape(-1)
    noise_at = _unit_noise_lookup(st, grids, unit_noise, hc.size, noise_before_truncate)
    power = np.zeros(2)

    def channel(x):
        y = pa_apply(x, point, ref_power)
        power[:] = (np.abs(x) ** 2).sum(), (np.abs(y) ** 2).sum()
        return np.convolve(hc, y)
    front = _sync_front(st, grids, noise_at, w_tx, None, snr_db, active, mask, noise_before_truncate, channel=channel)
    out = _sync_point(st, front, noise_at, w_rx, SyncPoint(0, 0.0, 1), bits_per_sc)
    return out[:8] + (power,) + ((out[8],) if with_y else ())


def _prepare_pa(points, ref_power, pairs):
    pts = [_pa_point(q) for q in points]
    if not pts:
        raise ValueError("at least one point is needed")
    ref = np.ascontiguousarray(np.atleast_1d(ref_power), dtype=np.float32)
    if ref.shape != (pairs,) or not (np.isfinite(ref) & (ref > 0)).all():
        raise ValueError("ref_power must hold %d finite positive powers" % pairs)
    return pts, ref


def rx_profile_pa_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, ref_power,
                       active=None, mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_pa_gpu``: the frames of ``rx_profile_host`` from the same Philox streams, each through
    ``frame_profile_pa`` for every point of ``points`` with the reference power ``ref_power`` [pairs] of the cell's window pair
    (single precision, as the GPU receives it); the labels and the noise of a frame are shared by its points.  Returns
    ``RxProfilePa``; with_near=True: also the number of ``near_decisions`` per point and cell [points, pairs, n_snr, n_ch]."""
    def arm(q):
        pts, ref = _prepare_pa(points, ref_power, q.w_tx.shape[0])

        def frame(p, s, c, cell, fr, grid):
            noise = gen_noise(q.noise_len, seed, cell, fr)
            return (frame_profile_pa(st, grid, noise, q.w_tx[p], q.w_rx[p], q.hc[c], pt, ref[p], q.snr[s], q.k, q.act, q.m, q.nbt)
                    for pt in pts)
        return (len(pts),), frame
    return _host_sweep(RxProfilePa, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                       active, mask, noise_before_truncate, with_near)


def rx_profile_pa_chunk_frames(st, syms, masked, n_points):
    """Frames one chunk of ``wofdm_rx_profile_pa`` holds (include/wofdm.h): ``rx_profile_sync_chunk_frames``' bytes plus one
    waveform per point; at most 65535."""
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms + st.tail_tx + syms * (st.sym_len - st.tail_tx),
                         n_points=n_points)


def rx_profile_pa_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, ref_power,
                      active=None, mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_pa``: ``rx_profile_gpu`` of the same arguments behind a memoryless power amplifier, for every point of
    ``points`` (``PaPoint`` or (model, ibo_db, smooth) tuples, at most ``_lib.PA_MAX_POINTS``) in ONE call -- the Tx chain runs
    once per frame, every point sees the same labels and noise --, per subcarrier and per data symbol.  ``ref_power`` [pairs]:
    the mean on-air power of a window pair's waveform the back-off counts from (``pa_ref_power``).  Returns ``RxProfilePa``;
    ``out`` (an earlier result of the same shape) is accumulated into.  No CPU fallback."""
    from . import _lib
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, ref = _prepare_pa(points, ref_power, prepared[0].shape[0])
    cpts = (_lib.PaPoint * len(pts))(*[_lib.PaPoint(q.model, q.ibo_db, q.smooth, 0) for q in pts])
    return _gpu_call("wofdm_rx_profile_pa", RxProfilePa, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                     noise_before_truncate, device, out, lead=(len(pts),), after_mask=(len(pts), cpts, ref.ctypes.data))


def pa_ref_power(st, bits_per_sc, syms, w_tx_pairs, seed, frame_offset, frames, active=None, mask=None, gpu=True, device=0):
    """The reference power of ``rx_profile_pa_gpu``: the mean on-air power per window pair [pairs] (float64) over the symbol
    periods of the frames [frame_offset, frame_offset + frames) that pair p transmits as cell p of ``tx_papr_gpu`` -- the sum of
    the periods' energies over frames * S * B samples, so the back-off counts from the same mean the PAPR histogram's axis
    counts from (the trailing tail_tx samples belong to no period).  gpu=True: from the {peak, energy} periods of
    ``tx_papr_gpu`` (as many calls as its ``periods`` output needs); gpu=False: from the host mirror ``timefreq.frame_papr`` on
    the same labels."""
    from . import _lib
    from . import timefreq as T
    w = _lib.f32(np.atleast_2d(w_tx_pairs))
    pairs, S, B = w.shape[0], int(syms), st.sym_len - st.tail_tx
    total = np.zeros(pairs, dtype=np.float64)
    if gpu:
        step = max(1, _lib.TX_PAPR_MAX_PERIODS // (pairs * S))
        for f0 in range(0, int(frames), step):
            per = T.tx_papr_gpu(st, bits_per_sc, S, w, seed, int(frame_offset) + f0, min(step, int(frames) - f0), active=active,
                                mask=mask, periods=True, device=device)[2]
            total += per[..., 1].astype(np.float64).sum(axis=(1, 2))
    else:
        tab = T.qam_table(bits_per_sc)
        on = np.ones(st.n_fft, dtype=bool) if active is None else np.asarray(active).reshape(-1) != 0
        m = None if mask is None else _lib.f32(np.asarray(mask).reshape(-1), (2 * st.sym_len - 1,))
        for p in range(pairs):
            grids = np.stack([tab[gen_labels(st.n_fft, bits_per_sc, S, seed, p, int(frame_offset) + f)] * on[None, :]
                              for f in range(int(frames))])
            total[p] = T.frame_papr(st, grids, w[p], m)[..., 1].sum()
    return total / (int(frames) * S * B)


# ---- under oscillator phase noise (wofdm_rx_profile_pn) ----

PnPoint = collections.namedtuple("PnPoint", "linewidth cpe_tracked", defaults=(0,))
PnPoint.__doc__ = """One oscillator of ``wofdm_rx_profile_pn``: linewidth (beta, the two-sided 3 dB width of its Lorentzian line
in subcarrier spacings, 0 <= beta <= 1, used as stored in single precision: the phase walks with variance 2 pi beta / n_fft per
sample), cpe_tracked (0: free-running; 1: a genie removes every symbol's common phase error)."""


def _pn_prepare(points):
    pts = [PnPoint(*q) for q in points]
    pts = [PnPoint(float(np.float32(q.linewidth)), int(q.cpe_tracked)) for q in pts]
    if not pts:
        raise ValueError("at least one point is needed")
    for q in pts:
        if not 0.0 <= q.linewidth <= 1.0 or q.cpe_tracked not in (0, 1):
            raise ValueError("a point needs 0 <= linewidth <= 1 and cpe_tracked in (0, 1): %r" % (q,))
    return pts


def gen_pn_increments(n, seed, cell, frame):
    """[n] float64: the phase-walk increments xi[0 ... n) of stream 3 of (seed, cell, frame), csrc/philox.h -- real unit
    normals, two per complex unit normal of the stream: complex index c = j >> 1 from block c >> 1, word pair c & 1 (the
    layout of ``gen_noise`` on stream 1), the real part for even j, the imaginary part for odd j; the uniforms in single
    precision as the kernels form them, Box-Muller in double."""
    n = int(n)
    nc = (n + 1) // 2
    w = _stream(seed, STREAM_PN, cell, frame, (nc + 1) // 2).reshape(-1, 2)[:nc]
    u1 = (w[:, 0].astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)
    u2 = (w[:, 1] >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)], axis=1).reshape(-1)[:n]


def pn_walk(n, seed, cell, frame):
    """[n] float64: the unit phase walk u[a] = xi[0] + ... + xi[a] of (seed, cell, frame), a < n -- what
    ``wofdm_pn_walk_kernel`` leaves for the n = S B on-air indices a receiver at timing 0 reads, up to the order of the fp64
    additions.  A point scales it by sigma = sqrt(2 pi linewidth / n_fft)."""
    return np.cumsum(gen_pn_increments(n, seed, cell, frame))


def _pn_turns(n_fft, u, a, q):
    """The phase of the prepared point q in turns, t [S, N + delta], where the walk u is read at the indices a [S, N + delta]
    (inside u), sigma / (2 pi), and the windows' mean walk ubar [S]"""
    turn = np.sqrt(q.linewidth / (2.0 * np.pi * n_fft))               # sigma / (2 pi), from beta as stored
    ubar = u[a[:, 0]] + np.mean(u[a] - u[a[:, :1]], axis=1)
    t = (u[a] - ubar[:, None] if q.cpe_tracked else u[a]) * turn
    return t, turn, ubar


def _pn_point(st, front, noise_at, w_rx, walk, point, bits_per_sc, with_cpe=False):
    """One point on a frame's shared part and its unit walk [S B]: ``_sync_point``'s outputs; with_cpe=True: also sigma and
    the windows' mean walk ubar [S]"""
    X, conv, g, on = front
    n, delta, gam = st.n_fft, st.tail_rx, st.prefix_rm
    S, B = X.shape[0], st.sym_len - st.tail_tx
    q = _pn_prepare([point])[0]
    u = np.asarray(walk, dtype=np.float64).reshape(-1)
    if u.size < S * B:
        raise ValueError("the walk holds %d samples, %d needed" % (u.size, S * B))
    a = (np.arange(S, dtype=np.int64) * B + gam)[:, None] + np.arange(n + delta, dtype=np.int64)[None, :]   # all in [0, S B)
    r = conv[a] + g * np.asarray(noise_at(a), dtype=np.complex128)
    t, turn, ubar = _pn_turns(n, u, a, q)
    out = _point_outputs(st, X, on, r * np.exp(2j * np.pi * (t - np.round(t))), w_rx, int(bits_per_sc))
    return out + (2.0 * np.pi * turn, ubar) if with_cpe else out


def frame_profile_pn(st, grids, unit_noise, w_tx, w_rx, h, walk, point, snr_db, bits_per_sc, active=None, mask=None,
                     noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_pn``: ``frame_profile`` with the receiver's oscillator
    phase a random walk.  walk [>= S B]: the frame's unit walk (``pn_walk``); sample m of symbol s sits at a = s B + prefix_rm
    + m and is multiplied, signal and noise, by e^{i sigma u[a]} (free-running) or e^{i sigma (u[a] - ubar_s)} (cpe_tracked),
    sigma^2 = 2 pi linewidth / n_fft, ubar_s the mean of u over the N + tail_rx samples under the symbol's window, before the Rx
    window; the noise gain never sees the phase and the pilot sees what the data sees.  unit_noise [noise_len] as
    ``frame_profile``'s.  Returns what ``frame_profile_sync`` returns: (bit_err [N], sym_err [N], err_power [N], xhat [S-1, N],
    y0 [N], bit_err_sym [S-1], sym_err_sym [S-1], err_power_sym [S-1]) -- the first five are ``frame_profile``'s, exactly, at
    linewidth = 0 under either flag --; with_y=True: Y [S, N], sigma and ubar [S] as a ninth to eleventh."""
    hc = np.asarray(h, dtype=np.complex128).reshape(-1)
    noise_at = _unit_noise_lookup(st, grids, unit_noise, hc.size, noise_before_truncate)
    front = _sync_front(st, grids, noise_at, w_tx, hc, snr_db, active, mask, noise_before_truncate)
    out = _pn_point(st, front, noise_at, w_rx, walk, point, bits_per_sc, with_cpe=True)
    return out if with_y else out[:8]


def rx_profile_pn_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points,
                       active=None, mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_pn_gpu``: the frames of ``rx_profile_host`` from the same Philox streams, each through
    ``frame_profile_pn`` for every point of ``points`` (``PnPoint`` or (linewidth, cpe_tracked) tuples); the Tx chain, the
    channel, the noise gain and the unit walk (stream 3) of a frame are shared by its points.  Returns ``RxProfileSync``;
    with_near=True: also the number of ``near_decisions`` per point and cell [points, pairs, n_snr, n_ch]."""
    def arm(q):
        pts = _pn_prepare(points)
        SB = q.S * (st.sym_len - st.tail_tx)

        def frame(p, s, c, cell, fr, grid):
            noise_at = _noise_lookup(gen_noise(max(q.noise_len, SB), seed, cell, fr))
            walk = pn_walk(SB, seed, cell, fr)
            front = _sync_front(st, grid, noise_at, q.w_tx[p], q.hc[c], q.snr[s], q.act, q.m, q.nbt)
            return (_pn_point(st, front, noise_at, q.w_rx[p], walk, pt, q.k)[:8] for pt in pts)
        return (len(pts),), frame
    return _host_sweep(RxProfileSync, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                       active, mask, noise_before_truncate, with_near)


def rx_profile_pn_chunk_frames(st, syms, masked, n_points):
    """Frames one chunk of ``wofdm_rx_profile_pn`` holds (include/wofdm.h): ``rx_profile_sync_chunk_frames``' bytes plus the
    frame's unit walk, S B doubles; at most 65535."""
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms, n_points=n_points,
                         per_frame_extra=syms * (st.sym_len - st.tail_tx))


def rx_profile_pn_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points,
                      active=None, mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_pn``: ``rx_profile_gpu`` of the same arguments under oscillator phase noise, for every point of
    ``points`` (``PnPoint`` or (linewidth, cpe_tracked) tuples, at most ``_lib.PN_MAX_POINTS``) in ONE call -- the Tx chain, the
    power pass and the phase walk run once per frame, every point sees the same labels, noise and unit walk --, per subcarrier
    and per data symbol.  Returns ``RxProfileSync``; ``out`` (an earlier result of the same shape) is accumulated into.  No
    CPU fallback."""
    import ctypes as C
    from . import _lib
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts = _pn_prepare(points)
    cpts = (_lib.PnPoint * len(pts))(*[_lib.PnPoint(q.linewidth, q.cpe_tracked, (C.c_int32 * 2)(0, 0)) for q in pts])
    return _gpu_call("wofdm_rx_profile_pn", RxProfileSync, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                     noise_before_truncate, device, out, lead=(len(pts),), after_mask=(len(pts), cpts))


# ---- the five impairments combined (wofdm_rx_profile_link) ----

LinkPoint = collections.namedtuple("LinkPoint", "pa track timing cfo cfo_tracked linewidth cpe_tracked aci",
                                   defaults=(None, None, 0, 0.0, 1, 0.0, 0, None))
LinkPoint.__doc__ = """One point of ``wofdm_rx_profile_link``, every field "off" by default: pa (a ``PaPoint`` or None: no amplifier),
track (index into the call's tracks, or None: the static channel h), timing, cfo, cfo_tracked (``SyncPoint``'s), linewidth,
cpe_tracked (``PnPoint``'s), aci ((delay, level_db) of the neighbour, or None: none on the air)."""

RxProfileLink = collections.namedtuple("RxProfileLink", RxProfilePa._fields)
RxProfileLink.__doc__ = """``RxProfilePa``'s fields with the points of ``wofdm_rx_profile_link`` on the leading axis; pa_power of a
point without an amplifier is {sum |x|^2, sum |x|^2}."""


def _link_prepare(st, points, n_tracks):
    """The points as the library reads them (single-precision values, None for what is off), checked against its limits"""
    B = st.sym_len - st.tail_tx
    pts = []
    for q in points:
        q = LinkPoint(*q)
        pa = None if q.pa is None else _pa_point(q.pa)
        track = None if q.track is None or int(q.track) == -1 else int(q.track)
        sync = _prepare_sync([(q.timing, q.cfo, q.cfo_tracked)])[0]
        pn = _pn_prepare([(q.linewidth, q.cpe_tracked)])[0]
        aci = None if q.aci is None else (int(q.aci[0]), float(np.float32(q.aci[1])))
        if track is not None and not 0 <= track < n_tracks:
            raise ValueError("a point's track must be None or in [0, %d): %r" % (n_tracks, q))
        if abs(sync.timing) >= B or not abs(sync.cfo) <= 4.0 or sync.cfo_tracked not in (0, 1):
            raise ValueError("a point needs |timing| < %d, |cfo| <= 4 and cfo_tracked in (0, 1): %r" % (B, q))
        if aci is not None and (not 0 <= aci[0] < B or not np.isfinite(aci[1])):
            raise ValueError("a point's neighbour needs 0 <= delay < %d and a finite level: %r" % (B, q))
        pts.append(LinkPoint(pa, track, sync.timing, sync.cfo, sync.cfo_tracked, pn.linewidth, pn.cpe_tracked, aci))
    if not pts:
        raise ValueError("at least one point is needed")
    return pts


def _link_front(st, grids, noise_at, w_tx, h, track, knot_step, pa, ref_power, snr_db, active, mask, noise_before_truncate):
    """``_sync_front`` of a point's waveform and channel -- ``pa_apply`` (pa None: x itself), then ``tv_conv`` with the track
    [n_knots, taps] or (None) conv with h --, and the two power sums of ``frame_profile_pa``"""
    power = np.zeros(2)

    def channel(x):
        y = x if pa is None else pa_apply(x, pa, ref_power)
        power[:] = (np.abs(x) ** 2).sum(), (np.abs(y) ** 2).sum()
        return np.convolve(np.asarray(h, dtype=np.complex128).reshape(-1), y) if track is None else tv_conv(track, knot_step, y)
    return _sync_front(st, grids, noise_at, w_tx, None, snr_db, active, mask, noise_before_truncate, channel=channel), power


def _link_walk_index(a, n):
    """The walk's index of the on-air index a: clamped onto [0, n), n = S B -- the oscillator holds its phase outside the frame"""
    return np.clip(np.asarray(a, dtype=np.int64), 0, n - 1)


def _link_point(st, front, power, noise_at, w_rx, walk, on_air, point, bits_per_sc):
    """One prepared point on its front: ``_sync_point`` with the neighbour ``on_air`` (``_aci_on_air`` at amplitude 1, or None)
    at the point's level and offset beside the received samples, and ``_pn_turns`` of the clamped walk behind the carrier
    offset's rotation.  Returns ``frame_profile_pa``'s nine outputs and Y."""
    S, B = front[0].shape[0], st.sym_len - st.tail_tx
    u = np.asarray(walk, dtype=np.float64).reshape(-1)
    if u.size < S * B:
        raise ValueError("the walk holds %d samples, %d needed" % (u.size, S * B))
    beside = None
    if point.aci is not None and on_air is not None:
        d, lvl = point.aci

        def beside(a):
            i = a + (B - d)
            return 10.0 ** (0.05 * lvl) * np.where((i >= 0) & (i < on_air.size), on_air[np.clip(i, 0, on_air.size - 1)], 0.0)

    def phase(a):
        t = _pn_turns(st.n_fft, u, _link_walk_index(a, S * B), PnPoint(point.linewidth, point.cpe_tracked))[0]
        return np.exp(2j * np.pi * (t - np.round(t)))
    out = _sync_point(st, front, noise_at, w_rx, SyncPoint(point.timing, point.cfo, point.cfo_tracked), bits_per_sc, beside, phase)
    return out[:8] + (power, out[8])


def frame_profile_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track=None, knot_step=None,
                       ref_power=None, aci_grids=None, aci_h=None, active=None, mask=None, noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_link``, composed of the arms' own mirrors: the Tx chain
    of ``frame_profile``; ``pa_apply`` (point.pa, ``ref_power``); ``tv_conv`` with ``track`` [n_knots, taps] -- the row of the
    call's tracks the point names, for the cell's channel -- or conv with h; the neighbour of ``frame_profile_aci`` (aci_grids [S
    + 1, N] through aci_h, None: h) at point.aci = (delay, level_db); Ps, Pn and g of the point's waveform and channel alone;
    the windows of ``frame_profile_sync`` at point.timing, its rotation, and then ``frame_profile_pn``'s with the unit walk
    ``walk`` [>= S B] read at clamp(a, 0, S B - 1), the tracked mean over the same clamped values.  noise_at(idx) as
    ``frame_profile_sync``'s.  Returns what ``frame_profile_pa`` returns: (bit_err [N], sym_err [N], err_power [N], xhat [S-1, N],
    y0 [N], bit_err_sym [S-1], sym_err_sym [S-1], err_power_sym [S-1], pa_power [2]); with_y=True: Y [S, N] as a tenth."""
    out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power, aci_grids,
                      aci_h, active, mask, noise_before_truncate)[1]
    return out if with_y else out[:9]


def _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power, aci_grids, aci_h,
                active, mask, noise_before_truncate):
    """The steps of ``frame_profile_link``: (the point's front (X, conv, g, on), ``_link_point``'s ten outputs)"""
    q = _link_prepare(st, [LinkPoint(*point)._replace(track=None)], 0)[0]
    if track is not None:
        q = q._replace(track=0)
    front, power = _link_front(st, grids, noise_at, w_tx, h, track, knot_step, q.pa, ref_power, snr_db, active, mask,
                               noise_before_truncate)
    on_air = None
    if q.aci is not None:
        if np.asarray(aci_grids).shape != (np.asarray(grids).shape[0] + 1, st.n_fft):
            raise ValueError("aci_grids must be [S + 1, %d]" % st.n_fft)
        on_air = _aci_on_air(st, aci_grids, w_tx, h if aci_h is None else aci_h, 0.0, mask)
    return front, _link_point(st, front, power, noise_at, w_rx, walk, on_air, q, bits_per_sc)


def _link_sides(st, hc, points, tracks, aci_active, aci_h, ref_power, pairs):
    """The prepared side arguments of a link call: points, tracks [n_tracks, n_ch, n_knots, taps] or None, the neighbour's
    allocation and channels or None, the reference powers [pairs] or None"""
    tr = None if tracks is None else _prepare_tracks(tracks)
    if tr is not None and (tr.shape[1] != hc.shape[0] or tr.shape[3] != hc.shape[1]):
        raise ValueError("tracks must have the channels and taps of h, %s" % (hc.shape,))
    pts = _link_prepare(st, points, 0 if tr is None else tr.shape[0])
    iact = hi = ref = None
    if any(q.aci is not None for q in pts):
        if aci_active is None:
            raise ValueError("a point has a neighbour: aci_active is needed")
        iact, hi = _prepare_aci(st, hc, aci_active, aci_h, 0, 0.0)[:2]
    if any(q.pa is not None and q.pa.model != PA_LINEAR for q in pts):
        if ref_power is None:
            raise ValueError("a point has an amplifier: ref_power is needed")
    if ref_power is not None:
        ref = _prepare_pa([PaPoint(PA_LINEAR, 0.0)], ref_power, pairs)[1]
    return pts, tr, iact, hi, ref


def rx_profile_link_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points,
                         tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                         noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_link_gpu``: the frames of ``rx_profile_host`` from the same Philox streams, each through
    ``frame_profile_link``'s steps for every point of ``points`` (``LinkPoint`` or tuples in its order); the labels, the noise,
    the unit walk and the neighbour of a frame are shared by its points, the waveform and the channel by the points with the
    same amplifier and track.  Returns ``RxProfileLink``; with_near=True: also the number of ``near_decisions`` per point and cell
    [points, pairs, n_snr, n_ch]."""
    from . import timefreq as T

    def arm(q):
        pts, tr, iact, hi, ref = _link_sides(st, q.hc, points, tracks, aci_active, aci_h, ref_power, q.w_tx.shape[0])
        B = st.sym_len - st.tail_tx
        nb = iact is not None and iact.any()
        # the sample indices a frame's points read, as one range (``rx_profile_sync_host``'s)
        lo = min(0, st.prefix_rm + min(pt.timing for pt in pts))
        hi_ = max(q.noise_len, (q.S - 1) * B + st.prefix_rm + max(pt.timing for pt in pts) + st.n_fft + st.tail_rx)
        tab = T.qam_table(q.k)

        def frame(p, s, c, cell, fr, grid):
            noise_at = _noise_lookup(gen_noise_at(np.arange(lo, hi_, dtype=np.int64), seed, cell, fr), lo)
            walk = pn_walk(q.S * B, seed, cell, fr)
            on_air = None
            if nb:
                igrid = tab[gen_labels(st.n_fft, q.k, q.S + 1, seed, cell, fr, STREAM_ACI)] * (iact != 0)[None, :]
                on_air = _aci_on_air(st, igrid, q.w_tx[p], q.hc[c] if hi is None else hi[c], 0.0, q.m)
            fronts = {}
            for pt in pts:
                key = (pt.pa, pt.track)
                if key not in fronts:
                    fronts[key] = _link_front(st, grid, noise_at, q.w_tx[p], q.hc[c], None if pt.track is None else tr[pt.track, c],
                                              knot_step, pt.pa, None if ref is None else ref[p], q.snr[s], q.act, q.m, q.nbt)
                yield _link_point(st, *fronts[key], noise_at, q.w_rx[p], walk, on_air, pt, q.k)[:9]
        return (len(pts),), frame
    return _host_sweep(RxProfileLink, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                       active, mask, noise_before_truncate, with_near)


def rx_profile_link_chunk_frames(st, syms, masked, n_points, neighbour):
    """Frames one chunk of ``wofdm_rx_profile_link`` holds (include/wofdm.h): ``rx_profile_pa_chunk_frames``' bytes plus the
    frame's unit walk, S B doubles, plus -- neighbour: a point has one on the air -- ``rx_profile_aci_chunk_frames``' buffers of
    the neighbour; at most 65535."""
    B = st.sym_len - st.tail_tx
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms + st.tail_tx + syms * B, n_points=n_points,
                         per_frame_extra=syms * B, neighbour=bool(neighbour))


def rx_profile_link_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, tracks=None,
                        knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                        noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_link``: ``rx_profile_gpu`` of the same arguments with the five impairments combined, for every point of
    ``points`` (``LinkPoint`` or tuples in its order, at most ``_lib.LINK_MAX_POINTS``) in ONE call -- amplifier, moving channel
    (``tracks`` [n_tracks, n_ch, n_knots, taps] and ``knot_step`` as ``rx_profile_doppler_gpu``'s), neighbour (``aci_active``,
    ``aci_h`` as ``rx_profile_aci_gpu``'s), receiver offsets and phase noise, each as its own call has it.  ``tracks``,
    ``aci_active`` and ``ref_power`` are needed only where a point uses them.  A point with one impairment on returns the bytes
    of that impairment's own call.  Returns ``RxProfileLink``; ``out`` (an earlier result of the same shape) is accumulated
    into.  No CPU fallback."""
    import ctypes as C
    from . import _lib
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    return _gpu_call("wofdm_rx_profile_link", RxProfileLink, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                     noise_before_truncate, device, out, lead=(len(pts),),
                     after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                 None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts))


# ---- soft decisions: bit LLRs and the achievable rate (wofdm_rx_profile_soft) ----

#: the default scales of ``rx_profile_soft_gpu``: the half-octave list 2^(1 - j / 2), j = 0 ... 15 (2 down to 0.011) -- the matched
#: scale runs from about 0.5 (the pilot's own noise) to 0.01 (where ISI dominates), and an octave grid gives up as much as 10 %
#: of the rate against a fine one
SOFT_SCALES = tuple(float(np.float32(2.0 ** (1.0 - 0.5 * j))) for j in range(16))

_SOFT_SUMS = RxProfilePa._fields[:-1] + ("bit_penalty", "bit_penalty_sym", "decisions")
#: the fields ``_host_sweep`` and ``_gpu_call`` add up for the soft call: ``RxProfileSoft`` without the scales
_RxSoftSums = collections.namedtuple("_RxSoftSums", _SOFT_SUMS)
RxProfileSoft = collections.namedtuple("RxProfileSoft", _SOFT_SUMS[:-1] + ("scales", "decisions"))
RxProfileSoft.__doc__ = """``RxProfileLink``'s fields, and bit_penalty (float64) [points, pairs, n_snr, n_ch, n_scales, N]: the sum
over a bin's decisions of sum_i log2(1 + exp(-(1 - 2 b_i) c_j Lambda_i)) for every scale c_j; bit_penalty_sym [points, pairs, n_snr,
n_ch, n_scales, S - 1]: the same sums over the loaded bins per data symbol; scales [n_scales] (float32, as the library received
them).  ``gmi_per_bin``, ``gmi_per_symbol`` and ``gmi`` turn them into rates."""


def _soft_scales(scales):
    from . import _lib
    sc = _lib.f32(np.asarray(SOFT_SCALES if scales is None else scales).reshape(-1))
    if not 1 <= sc.size <= _lib.SOFT_MAX_SCALES or not (np.isfinite(sc) & (sc > 0)).all():
        raise ValueError("1 to %d finite positive scales are needed" % _lib.SOFT_MAX_SCALES)
    return sc


def bit_llrs(bits_per_sc, xhat, nu=1.0):
    """The max-log bit metrics of the equalised values ``xhat`` (any shape), [..., k]: Lambda_i = (min over the constellation
    points whose bit i is 1 of |xhat - x|^2, less the same minimum over the points whose bit i is 0) / nu, i = 0 the top bit of
    the label -- positive for a 0.  Brute force over every point of ``timefreq.qam_table`` (the kernel forms the difference per
    axis); nu broadcasts against xhat."""
    from . import timefreq as T
    k = int(bits_per_sc)
    tab = T.qam_table(k)
    e = np.asarray(xhat, dtype=np.complex128)
    d = np.abs(e[..., None] - tab) ** 2                                # [..., 2^k]
    lab = np.arange(1 << k)
    out = np.empty(e.shape + (k,), dtype=np.float64)
    for i in range(k):
        one = ((lab >> (k - 1 - i)) & 1) != 0
        out[..., i] = d[..., one].min(axis=-1) - d[..., ~one].min(axis=-1)
    return out / np.asarray(nu, dtype=np.float64)[..., None]


def soft_penalties(bits_per_sc, X, xhat, nu, scales, on=None):
    """The penalties of ``wofdm_rx_profile_soft`` on a mirror's outputs: X [S - 1, N] the transmitted points of the data symbols,
    xhat [S - 1, N] the equalised values, nu [N] the noise variance the receiver assumes per bin, scales [n_scales]; on [N]: the
    loaded bins (None: all) -- nu and on may also be [S - 1, N], per symbol.  Returns pen [n_scales, S - 1, N] = sum_i log2(1 + exp(-(1 - 2 b_i) c_j Lambda_i)), evaluated as
    max(-z, 0) + log1p(exp(-|z|)) over ln 2, b_i the bits of X's label (``slice_labels``); 0 on unloaded bins."""
    k = int(bits_per_sc)
    X = np.asarray(X, dtype=np.complex128)
    on = np.ones((1, X.shape[-1]), dtype=bool) if on is None else np.atleast_2d(np.asarray(on) != 0)
    nu = np.where(on, np.atleast_2d(np.asarray(nu, dtype=np.float64)), 1.0)
    lab = slice_labels(k, X)
    sign = np.stack([1.0 - 2.0 * ((lab >> (k - 1 - i)) & 1) for i in range(k)], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z0 = sign * bit_llrs(k, np.where(on, xhat, 0.0), nu)                            # [S - 1, N, k]
        z = np.asarray(scales, dtype=np.float64).reshape(-1)[:, None, None, None] * z0[None]
        pen = ((np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z)))) / np.log(2.0)).sum(axis=-1)
    return np.where(on[None], pen, 0.0)


def _soft_outputs(st, front, out, w_rx, snr_db, bits_per_sc, scales, noise_before_truncate):
    """nu [N], bit penalties [n_scales, N] and symbol penalties [n_scales, S - 1] of a point of a frame: front = the point's (X,
    conv, g, on), out = ``_link_point``'s outputs (xhat fourth, Y last).  v = mean |conv|^2 10^(-snr / 10) over the samples the
    power pass reads -- which is g^2 Pn / NL --, W2 the sum of the window's squares, G = X_0 / Y_0."""
    X, conv, _, on = front
    S, B = X.shape[0], st.sym_len - st.tail_tx
    nl = conv.size if noise_before_truncate else S * B
    v = np.mean(np.abs(conv[:nl]) ** 2) * 10.0 ** (-0.1 * float(snr_db))
    w2 = float((np.asarray(w_rx, np.float64) ** 2).sum())
    Y0 = out[-1][0]
    with np.errstate(invalid="ignore", divide="ignore"):
        nu = np.where(on, np.abs(X[0] / np.where(on, Y0, 1.0)) ** 2 * v * w2, 0.0)
    pen = soft_penalties(bits_per_sc, X[1:], out[3], nu, scales, on)
    return nu, pen.sum(axis=1), pen.sum(axis=2)


def frame_profile_soft(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, scales=None, track=None,
                       knot_step=None, ref_power=None, aci_grids=None, aci_h=None, active=None, mask=None, noise_before_truncate=1,
                       with_y=False):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_soft``: ``frame_profile_link`` of the same arguments, and
    for the scales ``scales`` (None: ``SOFT_SCALES``) the penalties of include/wofdm.h's definition -- e = xhat, G = X_0 / Y_0,
    nu[n] = |G[n]|^2 v W2 with v = Ps / NL 10^(-snr / 10) of the point's waveform and channel and W2 = sum w_rx^2, the metrics of
    ``bit_llrs``, the sums of ``soft_penalties``.  Returns ``frame_profile_link``'s nine outputs, then nu [N], bit_penalty
    [n_scales, N] and bit_penalty_sym [n_scales, S - 1]; with_y=True: Y [S, N] as a thirteenth."""
    sc = _soft_scales(scales)
    front, out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power,
                             aci_grids, aci_h, active, mask, noise_before_truncate)
    soft = _soft_outputs(st, front, out, w_rx, snr_db, bits_per_sc, sc, noise_before_truncate)
    return out[:9] + soft + ((out[9],) if with_y else ())


def _soft_result(sums, scales):
    return RxProfileSoft(*sums[:-1], scales, sums.decisions)


def rx_profile_soft_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                         scales=None, tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None,
                         mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_soft_gpu``: ``rx_profile_link_host``'s frames and points (None: one all-off ``LinkPoint``),
    each also through ``frame_profile_soft``'s steps for the scales ``scales`` (None: ``SOFT_SCALES``).  Returns
    ``RxProfileSoft``; with_near=True: also the number of ``near_decisions`` per point and cell."""
    return _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                       knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near)


def _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver=None):
    """``rx_profile_soft_host``'s sweep; receiver(q: ``_Sweep``, n_points, scales) -> per point a function (front, out, p, s, c, f)
    -> the frame's tuple behind ``_link_point``'s outputs ``out`` in the place of the one-shot receiver's, (p, s, c) the cell's
    pair, SNR point and channel and f the frame's index in the call (``rx_profile_tracking_host``, ``rx_profile_coded_host``)"""
    from . import timefreq as T
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points

    def arm(q):
        pts, tr, iact, hi, ref = _link_sides(st, q.hc, points, tracks, aci_active, aci_h, ref_power, q.w_tx.shape[0])
        rec = None if receiver is None else receiver(q, len(pts), sc)
        B = st.sym_len - st.tail_tx
        nb = iact is not None and iact.any()
        lo = min(0, st.prefix_rm + min(pt.timing for pt in pts))
        hi_ = max(q.noise_len, (q.S - 1) * B + st.prefix_rm + max(pt.timing for pt in pts) + st.n_fft + st.tail_rx)
        tab = T.qam_table(q.k)

        def frame(p, s, c, cell, fr, grid):
            noise_at = _noise_lookup(gen_noise_at(np.arange(lo, hi_, dtype=np.int64), seed, cell, fr), lo)
            walk = pn_walk(q.S * B, seed, cell, fr)
            on_air = None
            if nb:
                igrid = tab[gen_labels(st.n_fft, q.k, q.S + 1, seed, cell, fr, STREAM_ACI)] * (iact != 0)[None, :]
                on_air = _aci_on_air(st, igrid, q.w_tx[p], q.hc[c] if hi is None else hi[c], 0.0, q.m)
            fronts = {}
            for i, pt in enumerate(pts):
                key = (pt.pa, pt.track)
                if key not in fronts:
                    fronts[key] = _link_front(st, grid, noise_at, q.w_tx[p], q.hc[c], None if pt.track is None else tr[pt.track, c],
                                              knot_step, pt.pa, None if ref is None else ref[p], q.snr[s], q.act, q.m, q.nbt)
                out = _link_point(st, *fronts[key], noise_at, q.w_rx[p], walk, on_air, pt, q.k)
                if rec is None:
                    yield out[:9] + _soft_outputs(st, fronts[key][0], out, q.w_rx[p], q.snr[s], q.k, sc, q.nbt)[1:]
                else:
                    yield rec[i](fronts[key][0], out, p, s, c, fr - int(frame_offset))
        return (len(pts),), frame
    res = _host_sweep(_RxSoftSums, arm, st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames,
                      active, mask, noise_before_truncate, with_near, n_scales=sc.size)
    return (_soft_result(res[0], sc), res[1]) if with_near else _soft_result(res, sc)


def rx_profile_soft_chunk_frames(st, syms, masked, n_points, neighbour, n_scales):
    """Frames one chunk of ``wofdm_rx_profile_soft`` holds (include/wofdm.h): ``rx_profile_link_chunk_frames``' bytes plus, per
    point and scale, the fp32 penalties of every data symbol's bins and the symbols' sums, 4 ((S - 1) N + S) bytes; at most 65535."""
    B = st.sym_len - st.tail_tx
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms + st.tail_tx + syms * B, n_points=n_points,
                         per_frame_extra=syms * B, neighbour=bool(neighbour),
                         extra_bytes=4 * int(n_points) * int(n_scales) * ((syms - 1) * st.n_fft + syms))


def rx_profile_soft_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                        scales=None, tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None,
                        mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_soft``: ``rx_profile_link_gpu`` of the same arguments -- its five outputs are that call's bytes -- and
    beside them the penalties of the max-log bit metrics for every scale of ``scales`` (None: ``SOFT_SCALES``; at most
    ``_lib.SOFT_MAX_SCALES``), per bin and per data symbol.  points=None is one all-off ``LinkPoint``.  Returns
    ``RxProfileSoft``; ``out`` (an earlier result of the same shape and scales) is accumulated into.  No CPU fallback."""
    import ctypes as C
    from . import _lib
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if not np.array_equal(out.scales, sc):
            raise ValueError("out has other scales")
        prev = _RxSoftSums(*out[:-2], out.decisions)
    res = _gpu_call("wofdm_rx_profile_soft", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data))
    return _soft_result(res, sc)


def _soft_rates(pen, dec, k):
    """k - pen / dec along the scale axis (-2 of pen) and its maximum: (rate, index of the scale), NaN / 0 where dec is 0"""
    dec = np.asarray(dec, dtype=np.float64)
    ok = dec > 0 if dec.ndim == 1 else (dec > 0)[..., None, :]         # (per point: the scale axis beside the others)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ok, int(k) - pen / np.where(dec > 0, dec, 1.0)[..., None, :], np.nan)
    bad = np.isnan(r).all(axis=-2)
    idx = np.where(bad, 0, np.argmax(np.where(np.isnan(r), -np.inf, r), axis=-2))
    return np.where(bad, np.nan, np.take_along_axis(r, idx[..., None, :], axis=-2)[..., 0, :]), idx


def gmi_per_bin(prof, bits_per_sc):
    """The achievable rate per subcarrier in bit per decision, k - bit_penalty / decisions at the scale that maximises it (every
    scale gives an achievable rate): (rate, scale index) [points, pairs, n_snr, n_ch, N]; NaN (index 0) on unloaded bins."""
    return _soft_rates(prof.bit_penalty, _decisions_like(prof.decisions, prof.bit_err), bits_per_sc)


def gmi_per_symbol(prof, bits_per_sc):
    """The same per data symbol over the loaded bins: (rate, scale index) [points, pairs, n_snr, n_ch, S - 1]"""
    n_sym = prof.bit_penalty_sym.shape[-1]
    if hasattr(prof, "decisions_sym"):
        return _soft_rates(prof.bit_penalty_sym, _decisions_like(prof.decisions_sym, prof.bit_err_sym), bits_per_sc)
    dec = np.full(n_sym, float(prof.decisions.astype(np.float64).sum()) / n_sym)
    return _soft_rates(prof.bit_penalty_sym, dec, bits_per_sc)


def gmi(prof, bits_per_sc, per_bin_scale=True):
    """The achievable rate of a cell in bit per decision, the mean over its loaded bins: per_bin_scale=True with every bin at its
    own best scale -- (rate [points, pairs, n_snr, n_ch], scale index [..., N], as ``gmi_per_bin``'s) --, False with one scale for
    the cell, the best for its total penalty -- (rate [...], scale index [...])."""
    per_point = prof.decisions.ndim == 2                               # (a tracking receiver's: the data bins are the call's)
    on = (prof.decisions > 0).any(axis=0) if per_point else prof.decisions > 0
    if per_bin_scale:
        r, idx = gmi_per_bin(prof, bits_per_sc)
        return r[..., on].mean(axis=-1), idx
    total = prof.decisions.astype(np.float64).sum(axis=-1)
    dec = _decisions_like(total[:, None], prof.bit_err) if per_point else np.array([float(total)])
    r, idx = _soft_rates(prof.bit_penalty.sum(axis=-1, keepdims=True), dec, bits_per_sc)
    return r[..., 0], idx[..., 0]


# ---- a receiver that tracks: comb pilots and a postamble (wofdm_rx_profile_tracking) ----

TrackingPoint = collections.namedtuple("TrackingPoint", "cpe post", defaults=(0, 0))
TrackingPoint.__doc__ = """The receiver of one point of ``wofdm_rx_profile_tracking``: cpe (1: the common phase of every data symbol
is estimated from the comb of pilot bins and removed), post (1: symbol S - 1 is a postamble, a second known symbol, and the
channel estimate is interpolated between the pilot and it; needs S >= 3).  (0, 0) is the one-shot receiver of every other call."""

RxProfileTracking = collections.namedtuple("RxProfileTracking", _SOFT_SUMS[:-1] + ("scales", "decisions_sym", "decisions"))
RxProfileTracking.__doc__ = """``RxProfileSoft``'s fields, with the decisions per point: decisions [points, N] = frames * (S - 1 -
post) on the data bins -- loaded and no pilot --, 0 on the others; decisions_sym [points, S - 1]: the decisions a data symbol
took per cell, frames * data bins, 0 for the postamble of a point with post."""


def pilot_comb(active, spacing, first=0):
    """[N] bool: every ``spacing``-th loaded bin of ``active`` [N] from the ``first`` loaded one on -- the comb of
    ``wofdm_rx_profile_tracking``"""
    act = np.asarray(active).reshape(-1) != 0
    if int(spacing) < 1 or int(first) < 0:
        raise ValueError("spacing must be >= 1 and first >= 0")
    out = np.zeros(act.size, dtype=bool)
    out[np.flatnonzero(act)[int(first)::int(spacing)]] = True
    return out


def tracking_equalise(X, Y, on, pilots, cpe, post):
    """The definition of include/wofdm.h (``wofdm_rx_profile_tracking``) in double precision.  X, Y [S, N]: the transmitted points
    and the DFT outputs of a frame; on [N]: the loaded bins; pilots [N] or None: the comb; cpe, post: the point's flags.  With t =
    s / (S - 1) for the symbols s = 1 ... S - 1:
      H0 = Y_0 / X_0 on the loaded bins; post: HL = Y_{S-1} / X_{S-1}, cL = sum_{n loaded} HL conj(H0), rho = cL / |cL| (1 if cL =
      0), Hh_s = H0 + t (HL conj(rho) - H0); else Hh_s = H0;
      cpe: c_s = sum_{p in pilots} Y_s[p] conj(Hh_s[p] X_s[p]), q_s = c_s / |c_s| (1 if c_s = 0); post alone: q_s = e^{i t arg rho};
      neither: q_s = 1;
      e = Y_s conj(q_s) / Hh_s.
    Returns (e [S - 1, N], Hh [S - 1, N], q [S - 1]): e is 0 where no decision is taken -- unloaded bins, pilot bins, and with
    post the row of symbol S - 1 --, Hh is 0 on the unloaded bins."""
    X, Y = np.asarray(X, dtype=np.complex128), np.asarray(Y, dtype=np.complex128)
    S, n = X.shape
    on = np.asarray(on).reshape(-1) != 0
    pil = np.zeros(n, dtype=bool) if pilots is None else np.asarray(pilots).reshape(-1) != 0
    if Y.shape != (S, n) or on.shape != (n,) or pil.shape != (n,) or (pil & ~on).any():
        raise ValueError("X, Y must be [S, N], on and pilots [N], and every pilot on a loaded bin")
    if cpe not in (0, 1) or post not in (0, 1) or (post and S < 3) or (cpe and not pil.any()):
        raise ValueError("flags must be 0 or 1, post needs S >= 3 and cpe a pilot bin")
    t = np.arange(1, S, dtype=np.float64) / (S - 1)
    H0 = np.zeros(n, dtype=np.complex128)
    H0[on] = Y[0, on] / X[0, on]
    Hh = np.tile(H0, (S - 1, 1))
    rho = 1.0 + 0.0j
    if post:
        HL = np.zeros(n, dtype=np.complex128)
        HL[on] = Y[S - 1, on] / X[S - 1, on]
        cL = (HL[on] * np.conj(H0[on])).sum()
        rho = cL / abs(cL) if cL != 0 else 1.0 + 0.0j
        Hh = H0[None, :] + t[:, None] * (HL * np.conj(rho) - H0)[None, :]
    q = np.ones(S - 1, dtype=np.complex128)
    if cpe:
        c = (Y[1:, pil] * np.conj(Hh[:, pil] * X[1:, pil])).sum(axis=1)
        q = np.where(c != 0, c / np.where(c != 0, np.abs(c), 1.0), 1.0)
    elif post:
        q = np.exp(1j * t * np.angle(rho))
    data = np.tile(on & ~pil, (S - 1, 1))
    if post:
        data[S - 2] = False
    e = np.zeros((S - 1, n), dtype=np.complex128)
    e[data] = (Y[1:] * np.conj(q)[:, None])[data] / Hh[data]
    return e, Hh, q


def _tracking_outputs(st, front, out, w_rx, snr_db, bits_per_sc, scales, noise_before_truncate, pilots, tp):
    """The frame's tuple of a point behind ``_link_point``'s outputs ``out`` (Y last), with ``tracking_equalise`` in the one-shot
    receiver's place: ``frame_profile_tracking``'s outputs.  The counters and the penalties are ``_point_outputs``' and
    ``_soft_outputs``' statements on e, with nu_s[n] = v W2 / |Hh_s[n]|^2."""
    X, conv, _, on = front
    k, S, B = int(bits_per_sc), X.shape[0], st.sym_len - st.tail_tx
    e, Hh, _ = tracking_equalise(X, out[-1], on, pilots, tp.cpe, tp.post)
    pil = np.zeros(on.size, dtype=bool) if pilots is None else np.asarray(pilots).reshape(-1) != 0
    data = np.tile(on & ~pil, (S - 1, 1))
    if tp.post:
        data[S - 2] = False
    d = np.where(data, slice_labels(k, X[1:]) ^ slice_labels(k, e), 0)
    bits = sum((d >> b) & 1 for b in range(k))
    err = np.where(data, np.abs(e - X[1:]) ** 2, 0.0)
    nl = conv.size if noise_before_truncate else S * B
    v = np.mean(np.abs(conv[:nl]) ** 2) * 10.0 ** (-0.1 * float(snr_db))
    w2 = float((np.asarray(w_rx, np.float64) ** 2).sum())
    Hd = np.where(data, Hh, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        nu = np.where(data, v * w2 / np.where(data, np.abs(Hh), 1.0) ** 2, 0.0)
    pen = soft_penalties(k, X[1:], e, nu, scales, data)
    return (bits.sum(axis=0).astype(np.uint64), (d != 0).sum(axis=0).astype(np.uint64), err.sum(axis=0), e, Hd,
            bits.sum(axis=1).astype(np.uint64), (d != 0).sum(axis=1).astype(np.uint64), err.sum(axis=1), out[8], pen.sum(axis=1),
            pen.sum(axis=2))


def _tracking_prepare(st, syms, n_points, tracking, pilots, act):
    """The tracking points (None: all (0, 0)), one per link point, and the comb [N] bool or None, checked as the library does"""
    tps = [TrackingPoint()] * n_points if tracking is None else [TrackingPoint(*(int(v) for v in TrackingPoint(*q))) for q in tracking]
    on = np.ones(st.n_fft, dtype=bool) if act is None else np.asarray(act).reshape(-1) != 0
    pil = None if pilots is None else np.ascontiguousarray(np.asarray(pilots).reshape(-1) != 0)
    if len(tps) != n_points:
        raise ValueError("%d tracking points for %d link points" % (len(tps), n_points))
    if pil is not None and (pil.shape != (st.n_fft,) or (pil & ~on).any()):
        raise ValueError("pilots must hold %d flags, each on a loaded bin" % st.n_fft)
    if not (on if pil is None else on & ~pil).any():
        raise ValueError("the comb leaves no data bin")
    for q in tps:
        if q.cpe not in (0, 1) or q.post not in (0, 1) or (q.post and int(syms) < 3) or (q.cpe and (pil is None or not pil.any())):
            raise ValueError("a tracking point needs flags 0 or 1, post S >= 3 and cpe a pilot bin: %r" % (q,))
    return tps, pil


def _tracking_decisions(st, syms, frames, act, pil, tps):
    """decisions [points, N] and decisions_sym [points, S - 1] of ``RxProfileTracking``"""
    on = np.ones(st.n_fft, dtype=bool) if act is None else np.asarray(act).reshape(-1) != 0
    data = on & ~pil if pil is not None else on
    S = int(syms)
    dec = np.stack([np.where(data, int(frames) * (S - 1 - q.post), 0) for q in tps]).astype(np.uint64)
    sym = np.full((len(tps), S - 1), int(frames) * int(data.sum()), dtype=np.uint64)
    for i, q in enumerate(tps):
        if q.post:
            sym[i, S - 2] = 0
    return dec, sym


def _tracking_result(sums, scales, dec, sym):
    return RxProfileTracking(*sums[:-1], scales, sym, dec)


def frame_profile_tracking(st, grids, noise_at, w_tx, w_rx, h, point, tracking, snr_db, bits_per_sc, walk, pilots=None, scales=None,
                           track=None, knot_step=None, ref_power=None, aci_grids=None, aci_h=None, active=None, mask=None,
                           noise_before_truncate=1, with_y=False):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_tracking``: ``frame_profile_soft``'s chain up to the DFT
    outputs, then ``tracking_equalise`` with the comb ``pilots`` and the point's ``tracking`` = (cpe, post), then the slicer, the
    error vector and the demapper on its e with nu_s[n] = v W2 / |Hh_s[n]|^2.  Returns (bit_err [N], sym_err [N], err_power [N], e
    [S-1, N], Hh [S-1, N] -- 0 where no decision is taken --, bit_err_sym [S-1], sym_err_sym [S-1], err_power_sym [S-1], pa_power
    [2], bit_penalty [n_scales, N], bit_penalty_sym [n_scales, S-1]); with_y=True: Y [S, N] as a twelfth."""
    sc = _soft_scales(scales)
    tps, pil = _tracking_prepare(st, np.asarray(grids).shape[0], 1, [tracking], pilots, active)
    front, out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power,
                             aci_grids, aci_h, active, mask, noise_before_truncate)
    res = _tracking_outputs(st, front, out, w_rx, snr_db, bits_per_sc, sc, noise_before_truncate, pil, tps[0])
    return res + ((out[9],) if with_y else ())


def rx_profile_tracking_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                             tracking=None, pilots=None, scales=None, tracks=None, knot_step=None, aci_active=None, aci_h=None,
                             ref_power=None, active=None, mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_tracking_gpu``: ``rx_profile_soft_host``'s frames and points, each through
    ``frame_profile_tracking``'s steps with the comb ``pilots`` [N] (None: none) and the point's ``TrackingPoint`` of ``tracking``
    (None: all (0, 0)).  Returns ``RxProfileTracking``; with_near=True: also the number of ``near_decisions`` per point and cell,
    the rule's weight being max_n |Hh_s| / |Hh_s[n]| per symbol."""
    held = {}

    def receiver(q, n_points, sc):
        tps, pil = _tracking_prepare(st, q.S, n_points, tracking, pilots, q.act)
        held.update(tps=tps, pil=pil, act=q.act)
        return [lambda front, out, p, s, c, f, tp=tp: _tracking_outputs(st, front, out, q.w_rx[p], q.snr[s], q.k, sc, q.nbt, pil, tp)
                for tp in tps]
    res = _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                      knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver)
    soft = res[0] if with_near else res
    dec, sym = _tracking_decisions(st, syms, frames, held["act"], held["pil"], held["tps"])
    prof = RxProfileTracking(*soft[:-1], sym, dec)
    return (prof, res[1]) if with_near else prof


def rx_profile_tracking_chunk_frames(st, syms, masked, n_points, neighbour, n_scales):
    """Frames one chunk of ``wofdm_rx_profile_tracking`` holds: ``rx_profile_soft_chunk_frames``' -- the receiver has no per-frame
    buffers of its own"""
    return rx_profile_soft_chunk_frames(st, syms, masked, n_points, neighbour, n_scales)


def rx_profile_tracking_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                            tracking=None, pilots=None, scales=None, tracks=None, knot_step=None, aci_active=None, aci_h=None,
                            ref_power=None, active=None, mask=None, noise_before_truncate=1, device=0, out=None):
    """``wofdm_rx_profile_tracking``: ``rx_profile_soft_gpu`` of the same arguments behind a receiver that tracks -- ``pilots`` [N]
    (None: no comb; ``pilot_comb``) and one ``TrackingPoint`` (or (cpe, post)) per point in ``tracking`` (None: all (0, 0), and
    then without a comb the soft call's bytes).  Pilot bins count nothing on any point, the postamble of a point with post
    nothing on that point.  Returns ``RxProfileTracking``; ``out`` (an earlier result of the same shape and scales) is
    accumulated into.  No CPU fallback."""
    import ctypes as C
    from . import _lib
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    tps, pil = _tracking_prepare(st, syms, len(pts), tracking, pilots, prepared[4])
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    ctps = (_lib.TrackingPoint * len(tps))(*[_lib.TrackingPoint(q.cpe, q.post, (C.c_int32 * 2)(0, 0)) for q in tps])
    pil8 = None if pil is None else np.ascontiguousarray(pil, dtype=np.uint8)
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if not np.array_equal(out.scales, sc):
            raise ValueError("out has other scales")
        prev = _RxSoftSums(*out[:-3], np.zeros(st.n_fft, dtype=np.uint64))
    res = _gpu_call("wofdm_rx_profile_tracking", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data, None if pil8 is None else pil8.ctypes.data, ctps))
    dec, sym = _tracking_decisions(st, syms, frames, prepared[4], pil, tps)
    if out is not None:
        if out.decisions.shape != dec.shape:
            raise ValueError("out has another shape")
        dec, sym = out.decisions + dec, out.decisions_sym + sym
    return _tracking_result(res, sc, dec, sym)


# ---- the coded link: 8-bit soft bits and a K = 7 Viterbi decoder (wofdm_rx_profile_coded, wofdm_viterbi_decode) ----

#: the rates of include/wofdm.h by index, and their puncturing patterns (A keeps, B keeps) by t mod period
CODE_RATES = ("1/2", "2/3", "3/4")
_PUNCTURE = (((1,), (1,)), ((1, 1), (1, 0)), ((1, 1, 0), (1, 0, 1)))
#: the default quantiser scale: it clamps 4-5 % of the soft bits on the mirror's 16-22 dB cells
LLR_SCALE = 0.25

RxProfileCoded = collections.namedtuple(
    "RxProfileCoded", RxProfileTracking._fields + ("info_err", "cw_err", "info_bits", "codewords", "rates", "llr_scale", "soft_bits"))
RxProfileCoded.__doc__ = """``RxProfileTracking``'s fields, and info_err, cw_err (uint64) [points, pairs, n_snr, n_ch, codes, S - 1]:
the decoded info-bit errors and codeword errors per data symbol; info_bits [codes]: T - 6 of each code; codewords [points, S - 1]:
the codewords a data symbol carried per cell (frames; 0 for the postamble of a point with post); rates [codes]; llr_scale;
soft_bits (int8) [pairs, n_snr, n_ch, frames, points, S - 1, N, 8] or None."""


def code_steps(rate, n_c):
    """T = wofdm_code_steps(rate, n_c) of include/wofdm.h: the largest T whose kept outputs number at most n_c"""
    rate, n_c = int(rate), int(n_c)
    if rate not in (0, 1, 2) or n_c < 0:
        raise ValueError("rate must be 0, 1 or 2 and n_c >= 0")
    if rate == 0:
        return n_c // 2
    if rate == 1:
        return 2 * (n_c // 3) + int(n_c % 3 == 2)
    return 3 * (n_c // 4) + (0, 0, 1, 2)[n_c % 4]


def _kept_index(rate, steps):
    """(ca, cb) [T]: the coded-stream index of A_t and of B_t, -1 where the pattern punctures it; and the kept outputs' number"""
    pa, pb = _PUNCTURE[int(rate)]
    ca, cb = np.full(steps, -1, dtype=np.int64), np.full(steps, -1, dtype=np.int64)
    c = 0
    for t in range(steps):
        if pa[t % len(pa)]:
            ca[t], c = c, c + 1
        if pb[t % len(pb)]:
            cb[t], c = c, c + 1
    return ca, cb, c


def _parity(v):
    v = np.asarray(v)
    return sum((v >> b) & 1 for b in range(7)) & 1


def default_interleaver(n_c):
    """perm [n_c]: the positions written row-wise into 17 columns and read column-wise -- 17 is coprime to k = 2, 4, 6, so
    neighbours of the coded stream land bins apart and on rotating bit significance"""
    return np.array([j for col in range(17) for j in range(col, int(n_c), 17)], dtype=np.int32)


def _check_perm(perm, n_c):
    if perm is None:
        return None
    p = np.ascontiguousarray(np.asarray(perm).reshape(-1), dtype=np.int32)
    if p.size != n_c or not np.array_equal(np.sort(p), np.arange(n_c)):
        raise ValueError("perm must be a permutation of 0 ... %d" % (n_c - 1))
    return p


def conv_encode(info, rate):
    """The K = 7, 133 / 171 code of include/wofdm.h: info [..., T - 6] bits -> the kept coded bits [..., n_kept] (uint8), A before
    B, t ascending, six zero tail bits appended"""
    info = np.asarray(info).astype(np.int64) & 1
    u = np.concatenate([info, np.zeros(info.shape[:-1] + (6,), dtype=np.int64)], axis=-1)
    steps = u.shape[-1]
    ca, cb, kept = _kept_index(rate, steps)
    out = np.zeros(u.shape[:-1] + (kept,), dtype=np.uint8)
    # bit j of the register r_t = (u_t << 6) | state is u_(t - 6 + j): every step's outputs at once, as parities of seven bits
    past = np.concatenate([np.zeros(u.shape[:-1] + (6,), dtype=np.int64), u], axis=-1)
    r = sum(past[..., j:j + steps] << j for j in range(7))
    out[..., ca[ca >= 0]] = _parity(r & 0o133)[..., ca >= 0]
    out[..., cb[cb >= 0]] = _parity(r & 0o171)[..., cb >= 0]
    return out


def viterbi_decode(soft, rate, perm=None):
    """The integer mirror of ``wofdm_viterbi_decode``, vectorised over the codewords: soft [n_cw, n_c] int8 (d > 0: a coded bit
    0), coded-stream index c reading soft[:, perm[c]] (None: c).  The metric is the sum of d over the kept outputs whose
    hypothesised bit is 1, int32; paths start in state 0 (2^30 on the others); the survivor is p0 = (s << 1) & 63 unless p1 = p0 | 1
    is strictly smaller; the traceback starts from state 0 at step T.  Returns (bits [n_cw, T] uint8, metric [n_cw] int32)."""
    soft = np.atleast_2d(np.asarray(soft)).astype(np.int32)
    n_cw, n_c = soft.shape
    steps = code_steps(rate, n_c)
    if steps < 7:
        raise ValueError("n_c=%d gives %d steps, at least 7 are needed" % (n_c, steps))
    p = _check_perm(perm, n_c)
    if p is not None:
        soft = soft[:, p]
    ca, cb, _ = _kept_index(rate, steps)
    ext = np.concatenate([soft, np.zeros((n_cw, 1), dtype=np.int32)], axis=1)        # (index -1: a punctured output, 0)
    d_a, d_b = ext[:, ca], ext[:, cb]
    s = np.arange(64)
    p0 = (s << 1) & 63
    p1, r0 = p0 | 1, ((s >> 5) << 6) | p0
    a0, b0 = _parity(r0 & 0o133).astype(np.int32), _parity(r0 & 0o171).astype(np.int32)   # (p1's pair is the complement)
    m = np.full((n_cw, 64), 1 << 30, dtype=np.int32)
    m[:, 0] = 0
    dec = np.empty((steps, n_cw, 64), dtype=bool)
    for t in range(steps):
        da, db = d_a[:, t:t + 1], d_b[:, t:t + 1]
        c0 = m[:, p0] + a0 * da + b0 * db
        c1 = m[:, p1] + (1 - a0) * da + (1 - b0) * db
        dec[t] = c1 < c0
        m = np.where(dec[t], c1, c0)
    state, rows = np.zeros(n_cw, dtype=np.int64), np.arange(n_cw)
    bits = np.empty((n_cw, steps), dtype=np.uint8)
    for t in range(steps - 1, -1, -1):
        bits[:, t] = state >> 5
        state = ((state << 1) & 63) | dec[t, rows, state]
    return bits, m[:, 0].astype(np.int32)


def viterbi_decode_gpu(soft, rate, perm=None, device=0):
    """``wofdm_viterbi_decode``: soft [n_cw, n_c] int8 -> (bits [n_cw, T] uint8, metric [n_cw] int32).  No CPU fallback."""
    from . import _lib
    soft = np.ascontiguousarray(np.atleast_2d(np.asarray(soft)), dtype=np.int8)
    n_cw, n_c = soft.shape
    steps = code_steps(rate, n_c)
    p = _check_perm(perm, n_c)
    bits = np.zeros((n_cw, max(steps, 1)), dtype=np.uint8)
    metric = np.zeros(n_cw, dtype=np.int32)
    _lib.check(_lib.load().wofdm_viterbi_decode(int(device), int(rate), n_c, None if p is None else p.ctypes.data, n_cw,
                                                soft.ctypes.data, bits.ctypes.data, metric.ctypes.data))
    return bits[:, :steps], metric


def soft_bits(z, llr_scale=LLR_SCALE):
    """The quantiser of include/wofdm.h on z = (1 - 2 b) Lambda (any shape): d = clip(rint(llr_scale z), -127, 127), round half
    even, int8, NaN -> 0.  Returns (d, llr_scale z unrounded)."""
    t = float(llr_scale) * np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(t), 0.0, np.clip(np.rint(t), -127.0, 127.0))
    return d.astype(np.int8), t


def _code_list(codes):
    rates = [int(r) for r in np.asarray((0,) if codes is None else codes).reshape(-1)]
    from . import _lib
    if not 1 <= len(rates) <= _lib.CODE_MAX or any(r not in (0, 1, 2) for r in rates):
        raise ValueError("1 to %d codes of rate 0, 1 or 2 are needed" % _lib.CODE_MAX)
    return rates


def _code_prepare(st, bits_per_sc, act, pil, codes, perm, llr_scale):
    """(rates, perm or None, pos [n_c]: the index 8 n + i of position j = r k + i in a symbol's soft bits [N, 8], T per code)"""
    rates = _code_list(codes)
    on = np.ones(st.n_fft, dtype=bool) if act is None else np.asarray(act).reshape(-1) != 0
    data = on & ~pil if pil is not None else on
    k = int(bits_per_sc)
    pos = (8 * np.flatnonzero(data)[:, None] + np.arange(k)[None, :]).reshape(-1)
    steps = [code_steps(r, pos.size) for r in rates]
    if min(steps) < 7:
        raise ValueError("%d coded bits per symbol give fewer than 7 steps" % pos.size)
    if not (np.isfinite(llr_scale) and llr_scale > 0):
        raise ValueError("llr_scale must be finite and positive")
    return rates, _check_perm(perm, pos.size), pos, steps


def _coded_z(st, front, res, w_rx, snr_db, bits_per_sc, noise_before_truncate, pil, tp):
    """z [S - 1, N, k] = (1 - 2 b_i) Lambda_i of the tracking mirror's outputs ``res`` (e fourth, Hh fifth) with nu_s[n] = v W2 /
    |Hh_s[n]|^2, 0 where no decision is taken; and the weight max_m |Hh_s[m]| / |Hh_s[n]| [S - 1, N] of the near rule"""
    X, conv, _, on = front
    k, S, B = int(bits_per_sc), X.shape[0], st.sym_len - st.tail_tx
    data = np.tile(on & ~pil if pil is not None else on, (S - 1, 1))
    if tp.post:
        data[S - 2] = False
    nl = conv.size if noise_before_truncate else S * B
    v = np.mean(np.abs(conv[:nl]) ** 2) * 10.0 ** (-0.1 * float(snr_db))
    w2 = float((np.asarray(w_rx, np.float64) ** 2).sum())
    mag = np.abs(res[4])
    with np.errstate(invalid="ignore", divide="ignore"):
        nu = np.where(data, v * w2 / np.where(data, mag, 1.0) ** 2, 1.0)
        weight = np.where(data, mag.max(axis=1, keepdims=True) / np.where(data, mag, 1.0), 0.0)
        lab = slice_labels(k, X[1:])
        sign = np.stack([1.0 - 2.0 * ((lab >> (k - 1 - i)) & 1) for i in range(k)], axis=-1)
        z = sign * bit_llrs(k, np.where(data, res[3], 0.0), nu)
    return np.where(data[..., None], z, 0.0), weight


def _decode_frame(d, tp, pos, perm, rates):
    """(info errors, codeword errors) [codes, S - 1] of a frame's soft bits d [S - 1, N, 8]: one codeword per data symbol, none
    on the postamble of a point with post"""
    S1 = d.shape[0]
    use = S1 - 1 if tp.post else S1
    info, cw = np.zeros((len(rates), S1), dtype=np.uint64), np.zeros((len(rates), S1), dtype=np.uint64)
    stream = d.reshape(S1, -1)[:use, pos]
    for j, r in enumerate(rates):
        bits, _ = viterbi_decode(stream, r, perm)
        info[j, :use] = bits[:, :bits.shape[1] - 6].sum(axis=1)
        cw[j, :use] = bits.any(axis=1)
    return info, cw


def frame_profile_coded(st, grids, noise_at, w_tx, w_rx, h, point, tracking, snr_db, bits_per_sc, walk, pilots=None, scales=None,
                        llr_scale=LLR_SCALE, perm=None, codes=None, track=None, knot_step=None, ref_power=None, aci_grids=None,
                        aci_h=None, active=None, mask=None, noise_before_truncate=1):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_coded``: ``frame_profile_tracking``'s outputs, then the
    soft bits d [S - 1, N, 8] (int8), llr_scale z unrounded [S - 1, N, k], the near rule's weight [S - 1, N], and the decoded
    info-bit and codeword errors [codes, S - 1] of ``viterbi_decode``."""
    sc = _soft_scales(scales)
    tps, pil = _tracking_prepare(st, np.asarray(grids).shape[0], 1, [tracking], pilots, active)
    rates, p, pos, _ = _code_prepare(st, bits_per_sc, active, pil, codes, perm, llr_scale)
    front, out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power,
                             aci_grids, aci_h, active, mask, noise_before_truncate)
    res = _tracking_outputs(st, front, out, w_rx, snr_db, bits_per_sc, sc, noise_before_truncate, pil, tps[0])
    z, weight = _coded_z(st, front, res, w_rx, snr_db, bits_per_sc, noise_before_truncate, pil, tps[0])
    d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
    d8[..., :z.shape[-1]], t = soft_bits(z, llr_scale)
    return res + (d8, t, weight) + _decode_frame(d8, tps[0], pos, p, rates)


def _coded_result(trk, info, cw, steps, tps, frames, rates, llr_scale, soft):
    S1 = trk.decisions_sym.shape[-1]
    words = np.full((len(tps), S1), int(frames), dtype=np.uint64)
    for i, q in enumerate(tps):
        if q.post:
            words[i, S1 - 1] = 0
    return RxProfileCoded(*trk, info, cw, np.array([t - 6 for t in steps], dtype=np.int64), words, tuple(rates), float(llr_scale), soft)


def rx_profile_coded_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                          tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, tracks=None,
                          knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                          noise_before_truncate=1, with_near=False, with_soft=False):
    """The host route of ``rx_profile_coded_gpu``: ``rx_profile_tracking_host``'s frames, points and arrays, each frame's z
    through ``soft_bits`` and every data symbol's codeword through ``viterbi_decode`` for the rates ``codes`` (None: rate 1/2).
    Returns ``RxProfileCoded`` (with_near: and the near decisions); with_soft=True keeps soft_bits, and the result carries two
    more arrays behind it in a tuple: llr_scale z unrounded [..., k] and the near rule's weight [..., S - 1, N]."""
    held = {}

    def receiver(q, n_points, sc):
        tps, pil = _tracking_prepare(st, q.S, n_points, tracking, pilots, q.act)
        rates, p, pos, steps = _code_prepare(st, q.k, q.act, pil, codes, perm, llr_scale)
        shape = (n_points, q.w_tx.shape[0], q.snr.size, q.hc.shape[0], len(rates), q.S - 1)
        held.update(tps=tps, pil=pil, act=q.act, rates=rates, steps=steps, info=np.zeros(shape, np.uint64), cw=np.zeros(shape, np.uint64))
        if with_soft:
            # [pairs, n_snr, n_ch, frames, points, S - 1, N, .]: the library's soft_bits, and beside it llr z and the weight
            lead = shape[1:4] + (int(frames), n_points, q.S - 1, st.n_fft)
            held.update(d=np.zeros(lead + (8,), np.int8), t=np.zeros(lead + (q.k,), np.float64), w=np.zeros(lead, np.float64))

        def one(i, tp):
            def run(front, out, p_, s_, c_, f_):
                res = _tracking_outputs(st, front, out, q.w_rx[p_], q.snr[s_], q.k, sc, q.nbt, pil, tp)
                z, weight = _coded_z(st, front, res, q.w_rx[p_], q.snr[s_], q.k, q.nbt, pil, tp)
                d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
                d8[..., :q.k], t = soft_bits(z, llr_scale)
                info, cw = _decode_frame(d8, tp, pos, p, rates)
                held["info"][i, p_, s_, c_] += info
                held["cw"][i, p_, s_, c_] += cw
                if with_soft:
                    held["d"][p_, s_, c_, f_, i], held["t"][p_, s_, c_, f_, i], held["w"][p_, s_, c_, f_, i] = d8, t, weight
                return res
            return run
        return [one(i, tp) for i, tp in enumerate(tps)]
    res = _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                      knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver)
    soft = res[0] if with_near else res
    dec, sym = _tracking_decisions(st, syms, frames, held["act"], held["pil"], held["tps"])
    trk = RxProfileTracking(*soft[:-1], sym, dec)
    prof = _coded_result(trk, held["info"], held["cw"], held["steps"], held["tps"], frames, held["rates"], llr_scale, held.get("d"))
    if with_soft:
        prof = (prof, held["t"], held["w"])
    return (prof, res[1]) if with_near else prof


def rx_profile_coded_chunk_frames(st, syms, masked, n_points, neighbour, n_scales):
    """Frames one chunk of ``wofdm_rx_profile_coded`` holds: ``rx_profile_tracking_chunk_frames``' bytes plus the soft bits, 8 (S -
    1) N bytes per point; at most 65535"""
    B = st.sym_len - st.tail_tx
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms + st.tail_tx + syms * B, n_points=n_points,
                         per_frame_extra=syms * B, neighbour=bool(neighbour),
                         extra_bytes=4 * int(n_points) * int(n_scales) * ((syms - 1) * st.n_fft + syms)
                         + 8 * int(n_points) * (syms - 1) * st.n_fft)


def rx_profile_coded_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                         tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, tracks=None,
                         knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                         noise_before_truncate=1, device=0, out=None, export=False):
    """``wofdm_rx_profile_coded``: ``rx_profile_tracking_gpu`` of the same arguments -- its fields are that call's bytes --, the
    demapper's z quantised to int8 with ``llr_scale``, and every data symbol's codeword decoded on the GPU for each rate of
    ``codes`` (None: rate 1/2) behind the interleaver ``perm`` (None: identity; ``default_interleaver``).  export=True also
    returns the soft bits.  Returns ``RxProfileCoded``; ``out`` (an earlier result of the same shape, scales and codes) is
    accumulated into (its soft bits are dropped).  No CPU fallback."""
    import ctypes as C
    from . import _lib
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    tps, pil = _tracking_prepare(st, syms, len(pts), tracking, pilots, prepared[4])
    rates, p, _, steps = _code_prepare(st, bits_per_sc, prepared[4], pil, codes, perm, llr_scale)
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    ctps = (_lib.TrackingPoint * len(tps))(*[_lib.TrackingPoint(q.cpe, q.post, (C.c_int32 * 2)(0, 0)) for q in tps])
    ccodes = (_lib.Code * len(rates))(*[_lib.Code(r, (C.c_int32 * 3)(0, 0, 0)) for r in rates])
    pil8 = None if pil is None else np.ascontiguousarray(pil, dtype=np.uint8)
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if not np.array_equal(out.scales, sc) or tuple(out.rates) != tuple(rates):
            raise ValueError("out has other scales or codes")
        prev = _RxSoftSums(*out[:9], np.zeros(st.n_fft, dtype=np.uint64))
    cells = (prepared[0].shape[0], prepared[3].size, prepared[2].shape[0])
    cerr = np.zeros((len(pts),) + cells + (len(rates), int(syms) - 1, 2), dtype=np.uint64)
    sb = np.zeros(cells + (int(frames), len(pts), int(syms) - 1, st.n_fft, 8), dtype=np.int8) if export else None
    res = _gpu_call("wofdm_rx_profile_coded", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data, None if pil8 is None else pil8.ctypes.data, ctps,
                                C.c_float(float(llr_scale)), None if p is None else p.ctypes.data, len(rates), ccodes),
                    behind=(cerr.ctypes.data, None if sb is None else sb.ctypes.data))
    dec, sym = _tracking_decisions(st, syms, frames, prepared[4], pil, tps)
    if out is not None:
        if out.decisions.shape != dec.shape:
            raise ValueError("out has another shape")
        dec, sym = out.decisions + dec, out.decisions_sym + sym
    prof = _coded_result(_tracking_result(res, sc, dec, sym), np.ascontiguousarray(cerr[..., 0]), np.ascontiguousarray(cerr[..., 1]),
                         steps, tps, frames, rates, llr_scale, sb)
    if out is not None:
        prof = prof._replace(info_err=out.info_err + prof.info_err, cw_err=out.cw_err + prof.cw_err,
                             codewords=out.codewords + prof.codewords)
    return prof


def _coded_rates(prof, err, per_word):
    err = err.astype(np.float64)                                       # [points, (pairs,) n_snr, n_ch, codes, S - 1]
    mid = (1,) * (err.ndim - 3)
    words = (prof.codewords.astype(np.float64).reshape((err.shape[0],) + mid + (1, err.shape[-1]))
             * np.asarray(per_word, np.float64).reshape((1,) + mid + (-1, 1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        per_sym = np.where(words > 0, err / np.where(words > 0, words, 1.0), np.nan)
        total = words.sum(axis=-1)
        per_cell = np.where(total > 0, err.sum(axis=-1) / np.where(total > 0, total, 1.0), np.nan)
    return per_sym, per_cell


def coded_ber(prof):
    """The decoded info-bit error rate: (per data symbol [points, pairs, n_snr, n_ch, codes, S - 1], per cell [..., codes]); NaN
    where a symbol carried no codeword"""
    return _coded_rates(prof, prof.info_err, prof.info_bits)


def coded_cwer(prof):
    """The codeword error rate, shaped as ``coded_ber``'s"""
    return _coded_rates(prof, prof.cw_err, np.ones(len(prof.rates)))


# ---- the coded link with frame-spanning codewords (wofdm_rx_profile_coded_frame, wofdm_viterbi_decode_long) ----

RxProfileCodedFrame = collections.namedtuple(
    "RxProfileCodedFrame", RxProfileTracking._fields + ("info_err", "cw_err", "info_bits", "codewords", "rates", "llr_scale", "sym_rot",
                                                        "soft_bits"))
RxProfileCodedFrame.__doc__ = """``RxProfileTracking``'s fields, and info_err, cw_err (uint64) [points, pairs, n_snr, n_ch, codes]: the
decoded info-bit errors and codeword errors of the frames' codewords; info_bits [points, codes]: T - 6 of each code over the point's
data symbols; codewords [points]: the codewords per cell (frames); rates [codes]; llr_scale; sym_rot; soft_bits (int8) [pairs,
n_snr, n_ch, frames, points, S - 1, N, 8] or None."""


def default_sym_rot(n_c, s_d):
    """The rotation that spreads a frame's symbols evenly over the interleaver's span: n_c // s_d"""
    return int(n_c) // int(s_d)


def frame_interleaver(n_c, s_d, sym_rot, perm=None):
    """The frame interleaver of include/wofdm.h: (j, position) [n_c s_d] -- coded-stream index c sits in data symbol 1 + j, j = c
    mod s_d, at the symbol's position perm[(c div s_d + j sym_rot) mod n_c] (perm None: the identity).  sym_rot >= 0 counts
    modulo n_c (``default_sym_rot`` of one symbol is n_c, which is 0); the library takes [0, n_c) only."""
    n_c, s_d, sym_rot = int(n_c), int(s_d), int(sym_rot)
    if n_c < 1 or s_d < 1 or sym_rot < 0:
        raise ValueError("n_c and s_d must be >= 1 and sym_rot >= 0")
    p = _check_perm(perm, n_c)
    c = np.arange(n_c * s_d, dtype=np.int64)
    j, q = c % s_d, c // s_d
    at = (q + j * sym_rot) % n_c
    return j, (at if p is None else p[at].astype(np.int64))


def viterbi_decode_long_gpu(soft, rate, perm=None, device=0):
    """``wofdm_viterbi_decode_long``: ``viterbi_decode_gpu`` for codewords of up to 2^20 steps, the same bits and metric.  No CPU
    fallback."""
    from . import _lib
    soft = np.ascontiguousarray(np.atleast_2d(np.asarray(soft)), dtype=np.int8)
    n_cw, n_c = soft.shape
    steps = code_steps(rate, n_c)
    p = _check_perm(perm, n_c)
    bits = np.zeros((n_cw, max(steps, 1)), dtype=np.uint8)
    metric = np.zeros(n_cw, dtype=np.int32)
    _lib.check(_lib.load().wofdm_viterbi_decode_long(int(device), int(rate), n_c, None if p is None else p.ctypes.data, n_cw,
                                                     soft.ctypes.data, bits.ctypes.data, metric.ctypes.data))
    return bits[:, :steps], metric


def _frame_code_prepare(st, bits_per_sc, syms, act, pil, tps, codes, perm, llr_scale, sym_rot):
    """(rates, perm or None, pos [n_c] as ``_code_prepare``'s, sym_rot, T [points, codes] over each point's data symbols)"""
    from . import _lib
    rates = _code_list(codes)
    on = np.ones(st.n_fft, dtype=bool) if act is None else np.asarray(act).reshape(-1) != 0
    data = on & ~pil if pil is not None else on
    pos = (8 * np.flatnonzero(data)[:, None] + np.arange(int(bits_per_sc))[None, :]).reshape(-1)
    if not (np.isfinite(llr_scale) and llr_scale > 0):
        raise ValueError("llr_scale must be finite and positive")
    rot = default_sym_rot(pos.size, max(int(syms) - 1, 1)) % pos.size if sym_rot is None else int(sym_rot)
    if not 0 <= rot < pos.size:
        raise ValueError("sym_rot must be in [0, %d)" % pos.size)
    steps = np.array([[code_steps(r, pos.size * (int(syms) - 1 - int(q.post))) if int(syms) - 1 - int(q.post) >= 1 else 0
                       for r in rates] for q in tps], dtype=np.int64).reshape(len(tps), len(rates))
    used = steps[steps > 0]
    if used.size and used.min() < 7:
        raise ValueError("%d coded bits per symbol give a codeword of fewer than 7 steps" % pos.size)
    if used.size and used.max() > _lib.CODE_LONG_MAX_STEPS:
        raise ValueError("a codeword of more than %d steps" % _lib.CODE_LONG_MAX_STEPS)
    return rates, _check_perm(perm, pos.size), pos, rot, steps


def frame_codewords(d, post, pos, perm, sym_rot):
    """The frames' codewords of soft bits d [..., S - 1, N, 8] (int8) as the decoder reads them: [..., n_c S_d], S_d = S - 1 - post,
    gathered through ``frame_interleaver``; pos: the index 8 n + i of a symbol's position (``_code_prepare``)"""
    d = np.asarray(d)
    S1 = d.shape[-3]
    s_d = S1 - int(bool(post))
    j, at = frame_interleaver(pos.size, s_d, sym_rot, perm)
    return d.reshape(d.shape[:-3] + (S1, -1))[..., j, np.asarray(pos)[at]]


def _decode_frame_long(d, tp, pos, perm, rates, sym_rot):
    """(info errors, codeword errors) [codes] of a frame's soft bits d [S - 1, N, 8]: one codeword over the point's data symbols"""
    info, cw = np.zeros(len(rates), dtype=np.uint64), np.zeros(len(rates), dtype=np.uint64)
    if d.shape[0] - int(bool(tp.post)) < 1:
        return info, cw
    word = frame_codewords(d, tp.post, pos, perm, sym_rot)[None]
    for i, r in enumerate(rates):
        bits, _ = viterbi_decode(word, r)
        info[i], cw[i] = bits[0, :bits.shape[1] - 6].sum(), bits[0].any()
    return info, cw


def frame_profile_coded_frame(st, grids, noise_at, w_tx, w_rx, h, point, tracking, snr_db, bits_per_sc, walk, pilots=None, scales=None,
                              llr_scale=LLR_SCALE, perm=None, codes=None, sym_rot=None, track=None, knot_step=None, ref_power=None,
                              aci_grids=None, aci_h=None, active=None, mask=None, noise_before_truncate=1):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_coded_frame``: ``frame_profile_coded``'s outputs through the
    near rule's weight, then the decoded info-bit and codeword errors [codes] of the frame's one codeword (``viterbi_decode``)."""
    sc = _soft_scales(scales)
    syms = np.asarray(grids).shape[0]
    tps, pil = _tracking_prepare(st, syms, 1, [tracking], pilots, active)
    rates, p, pos, rot, _ = _frame_code_prepare(st, bits_per_sc, syms, active, pil, tps, codes, perm, llr_scale, sym_rot)
    front, out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power,
                             aci_grids, aci_h, active, mask, noise_before_truncate)
    res = _tracking_outputs(st, front, out, w_rx, snr_db, bits_per_sc, sc, noise_before_truncate, pil, tps[0])
    z, weight = _coded_z(st, front, res, w_rx, snr_db, bits_per_sc, noise_before_truncate, pil, tps[0])
    d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
    d8[..., :z.shape[-1]], t = soft_bits(z, llr_scale)
    return res + (d8, t, weight) + _decode_frame_long(d8, tps[0], pos, p, rates, rot)


def _coded_frame_result(trk, info, cw, steps, frames, rates, llr_scale, sym_rot, soft):
    return RxProfileCodedFrame(*trk, info, cw, np.maximum(steps - 6, 0), np.full(steps.shape[0], int(frames), dtype=np.uint64),
                               tuple(rates), float(llr_scale), int(sym_rot), soft)


def rx_profile_coded_frame_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                                tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, sym_rot=None,
                                tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                                noise_before_truncate=1, with_near=False, with_soft=False):
    """The host route of ``rx_profile_coded_frame_gpu``: ``rx_profile_coded_host``'s frames, points, arrays and soft bits, each
    (frame, point)'s one codeword through ``frame_interleaver`` and ``viterbi_decode`` for the rates ``codes`` (None: rate 1/2);
    sym_rot None: ``default_sym_rot`` over S - 1 symbols.  Returns ``RxProfileCodedFrame`` (with_near: and the near decisions);
    with_soft as in ``rx_profile_coded_host``."""
    held = {}

    def receiver(q, n_points, sc):
        tps, pil = _tracking_prepare(st, q.S, n_points, tracking, pilots, q.act)
        rates, p, pos, rot, steps = _frame_code_prepare(st, q.k, q.S, q.act, pil, tps, codes, perm, llr_scale, sym_rot)
        shape = (n_points, q.w_tx.shape[0], q.snr.size, q.hc.shape[0], len(rates))
        held.update(tps=tps, pil=pil, act=q.act, rates=rates, steps=steps, rot=rot, info=np.zeros(shape, np.uint64),
                    cw=np.zeros(shape, np.uint64))
        if with_soft:
            lead = shape[1:4] + (int(frames), n_points, q.S - 1, st.n_fft)
            held.update(d=np.zeros(lead + (8,), np.int8), t=np.zeros(lead + (q.k,), np.float64), w=np.zeros(lead, np.float64))

        def one(i, tp):
            def run(front, out, p_, s_, c_, f_):
                res = _tracking_outputs(st, front, out, q.w_rx[p_], q.snr[s_], q.k, sc, q.nbt, pil, tp)
                z, weight = _coded_z(st, front, res, q.w_rx[p_], q.snr[s_], q.k, q.nbt, pil, tp)
                d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
                d8[..., :q.k], t = soft_bits(z, llr_scale)
                info, cw = _decode_frame_long(d8, tp, pos, p, rates, rot)
                held["info"][i, p_, s_, c_] += info
                held["cw"][i, p_, s_, c_] += cw
                if with_soft:
                    held["d"][p_, s_, c_, f_, i], held["t"][p_, s_, c_, f_, i], held["w"][p_, s_, c_, f_, i] = d8, t, weight
                return res
            return run
        return [one(i, tp) for i, tp in enumerate(tps)]
    res = _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                      knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver)
    soft = res[0] if with_near else res
    dec, sym = _tracking_decisions(st, syms, frames, held["act"], held["pil"], held["tps"])
    trk = RxProfileTracking(*soft[:-1], sym, dec)
    prof = _coded_frame_result(trk, held["info"], held["cw"], held["steps"], frames, held["rates"], llr_scale, held["rot"], held.get("d"))
    if with_soft:
        prof = (prof, held["t"], held["w"])
    return (prof, res[1]) if with_near else prof


def rx_profile_coded_frame_chunk_frames(st, bits_per_sc, syms, masked, n_points, neighbour, n_scales, n_data_bins, codes=(0,), post=False):
    """Frames one chunk of ``wofdm_rx_profile_coded_frame`` holds: ``rx_profile_coded_chunk_frames``' bytes plus the survivor
    history, 512 ceil(T_max / 64) bytes per point, T_max the longest codeword: the largest rate of ``codes`` over S - 1 data symbols
    (post=True: every point has a postamble, S - 2) of n_data_bins bins; at most 65535"""
    B = st.sym_len - st.tail_tx
    n_f = int(bits_per_sc) * int(n_data_bins) * (int(syms) - 1 - int(bool(post)))
    t_max = max(code_steps(r, n_f) for r in _code_list(codes))
    return _chunk_frames(st, syms, masked, per_point=st.n_fft + syms + st.tail_tx + syms * B, n_points=n_points,
                         per_frame_extra=syms * B, neighbour=bool(neighbour),
                         extra_bytes=4 * int(n_points) * int(n_scales) * ((syms - 1) * st.n_fft + syms)
                         + 8 * int(n_points) * (syms - 1) * st.n_fft + 512 * int(n_points) * ((t_max + 63) // 64))


def rx_profile_coded_frame_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                               tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, sym_rot=None,
                               tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                               noise_before_truncate=1, device=0, out=None, export=False):
    """``wofdm_rx_profile_coded_frame``: ``rx_profile_coded_gpu``'s frames, tracking fields and soft bits -- that call's bytes --,
    and per point and frame ONE codeword over the point's data symbols, interleaved by ``frame_interleaver`` with ``perm`` and
    ``sym_rot`` (None: ``default_sym_rot`` over S - 1 symbols) and decoded on the GPU for each rate of ``codes`` (None: rate 1/2).
    export=True also returns the soft bits.  Returns ``RxProfileCodedFrame``; ``out`` (an earlier result of the same shape, scales,
    codes and sym_rot) is accumulated into (its soft bits are dropped).  No CPU fallback."""
    import ctypes as C
    from . import _lib
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    tps, pil = _tracking_prepare(st, syms, len(pts), tracking, pilots, prepared[4])
    rates, p, _, rot, steps = _frame_code_prepare(st, bits_per_sc, syms, prepared[4], pil, tps, codes, perm, llr_scale, sym_rot)
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    ctps = (_lib.TrackingPoint * len(tps))(*[_lib.TrackingPoint(q.cpe, q.post, (C.c_int32 * 2)(0, 0)) for q in tps])
    ccodes = (_lib.Code * len(rates))(*[_lib.Code(r, (C.c_int32 * 3)(0, 0, 0)) for r in rates])
    pil8 = None if pil is None else np.ascontiguousarray(pil, dtype=np.uint8)
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if not np.array_equal(out.scales, sc) or tuple(out.rates) != tuple(rates) or out.sym_rot != rot:
            raise ValueError("out has other scales, codes or sym_rot")
        prev = _RxSoftSums(*out[:9], np.zeros(st.n_fft, dtype=np.uint64))
    cells = (prepared[0].shape[0], prepared[3].size, prepared[2].shape[0])
    ferr = np.zeros((len(pts),) + cells + (len(rates), 2), dtype=np.uint64)
    sb = np.zeros(cells + (int(frames), len(pts), int(syms) - 1, st.n_fft, 8), dtype=np.int8) if export else None
    res = _gpu_call("wofdm_rx_profile_coded_frame", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data, None if pil8 is None else pil8.ctypes.data, ctps,
                                C.c_float(float(llr_scale)), None if p is None else p.ctypes.data, len(rates), ccodes, int(rot)),
                    behind=(ferr.ctypes.data, None if sb is None else sb.ctypes.data))
    dec, sym = _tracking_decisions(st, syms, frames, prepared[4], pil, tps)
    if out is not None:
        if out.decisions.shape != dec.shape:
            raise ValueError("out has another shape")
        dec, sym = out.decisions + dec, out.decisions_sym + sym
    prof = _coded_frame_result(_tracking_result(res, sc, dec, sym), np.ascontiguousarray(ferr[..., 0]),
                               np.ascontiguousarray(ferr[..., 1]), steps, frames, rates, llr_scale, rot, sb)
    if out is not None:
        prof = prof._replace(info_err=out.info_err + prof.info_err, cw_err=out.cw_err + prof.cw_err,
                             codewords=out.codewords + prof.codewords)
    return prof


def coded_frame_ber(prof):
    """The decoded info-bit error rate of the frames' codewords [points, pairs, n_snr, n_ch, codes]; NaN where a point carried no
    codeword"""
    bits = (prof.codewords.astype(np.float64)[:, None] * prof.info_bits.astype(np.float64)).reshape(
        (prof.info_err.shape[0],) + (1,) * (prof.info_err.ndim - 2) + (-1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bits > 0, prof.info_err.astype(np.float64) / np.where(bits > 0, bits, 1.0), np.nan)


def coded_fer(prof):
    """The frame (codeword) error rate, shaped as ``coded_frame_ber``'s"""
    words = (prof.codewords.astype(np.float64)[:, None] * (prof.info_bits > 0)).reshape(
        (prof.cw_err.shape[0],) + (1,) * (prof.cw_err.ndim - 2) + (-1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(words > 0, prof.cw_err.astype(np.float64) / np.where(words > 0, words, 1.0), np.nan)


# ---- the coded link with a quasi-cyclic LDPC code (wofdm_rx_profile_ldpc, wofdm_ldpc_decode) ----

#: the iterations a code runs at most where none are given
LDPC_MAX_ITER = 30

RxProfileLdpc = collections.namedtuple(
    "RxProfileLdpc", RxProfileTracking._fields + ("info_err", "cw_err", "unconverged", "iterations", "info_bits", "codewords", "codes",
                                                  "llr_scale", "sym_rot", "soft_bits"))
RxProfileLdpc.__doc__ = """``RxProfileTracking``'s fields, and info_err, cw_err, unconverged, iterations (uint64) [points, pairs, n_snr,
n_ch, codes]: the decoded info-bit errors, the codewords with one, the codewords whose syndrome never vanished and the iterations
run, summed over the frames' codewords; info_bits [points, codes]: K of each code at the point's word length; codewords [points]:
the codewords per cell (frames times W); codes [codes]: (J, L, max_iter); llr_scale; sym_rot; soft_bits (int8) [pairs, n_snr, n_ch,
frames, points, S - 1, N, 8] or None."""


def ldpc_lift(J, L, n):
    """The lift of include/wofdm.h: the smallest prime Z >= max(L, ceil(n / L)) whose multiplicative order of 2 is at least L.
    ValueError outside 3 <= J <= 6, J < L <= 24, n >= 1, or where K = (L - J) Z - (L Z - n) < 1."""
    J, L, n = int(J), int(L), int(n)
    if not (3 <= J <= 6 and J < L <= 24 and n >= 1):
        raise ValueError("a code needs 3 <= J <= 6, J < L <= 24 and n >= 1")
    Z = max(L, -(-n // L))
    while True:
        if Z >= 3 and all(Z % d for d in range(2, int(Z ** 0.5) + 1)) and all(pow(2, k, Z) != 1 for k in range(1, L)):
            break
        Z += 1
    if (L - J) * Z - (L * Z - n) < 1:
        raise ValueError("(%d, %d) over %d positions has no information bit" % (J, L, n))
    return Z


def ldpc_edges(J, L, n):
    """(Z, [layer i: int64 [L - i, Z]]): the variable that edge e of check i Z + r joins, (i + e) Z + (r + s(i, i + e)) mod Z with
    s(i, j) = (i 2^j) mod Z -- the check matrix of include/wofdm.h, layer by layer, edges in column order"""
    Z = ldpc_lift(J, L, n)
    r = np.arange(Z, dtype=np.int64)
    return Z, [np.stack([j * Z + (r + (i * pow(2, j, Z)) % Z) % Z for j in range(i, int(L))]) for i in range(int(J))]


def ldpc_encode(info, J, L, n):
    """The encoder of include/wofdm.h: info [..., K] bits -> the codeword's n transmitted bits [..., n] (uint8), the information
    bits at J Z ... n - 1 and the shortened positions zero; back-substitution from block row J - 1 up to 0"""
    Z, idx = ldpc_edges(J, L, n)
    info = np.asarray(info).astype(np.uint8) & 1
    if info.shape[-1] != n - J * Z:
        raise ValueError("the code has K = %d information bits" % (n - J * Z))
    x = np.zeros(info.shape[:-1] + (int(L) * Z,), dtype=np.uint8)
    x[..., J * Z:n] = info
    for i in range(int(J) - 1, -1, -1):
        x[..., idx[i][0]] = x[..., idx[i][1:]].sum(axis=-2, dtype=np.int64) & 1
    return x[..., :n]


def ldpc_decode_at(soft, J, L, stops, perm=None):
    """``ldpc_decode`` at several max_iter in one run: {max_iter: (bits, iters, converged)} for every max_iter of ``stops`` -- a
    decoder stopped at M is the longer run's state after M iterations, the words that converged earlier frozen"""
    soft = np.atleast_2d(np.asarray(soft)).astype(np.int16)
    n_cw, n = soft.shape
    J, L = int(J), int(L)
    Z, idx = ldpc_edges(J, L, n)
    stops = sorted({int(m) for m in stops})
    if not stops or stops[0] < 1 or stops[-1] > 64:
        raise ValueError("max_iter must be 1 ... 64")
    p = _check_perm(perm, n)
    if p is not None:
        soft = soft[:, p]
    Q = np.full((n_cw, L * Z), 127, dtype=np.int16)
    Q[:, :n] = soft
    R = [np.zeros((n_cw, L - i, Z), dtype=np.int16) for i in range(J)]
    iters, conv, live, res = np.zeros(n_cw, dtype=np.int32), np.zeros(n_cw, dtype=bool), np.arange(n_cw), {}
    for it in range(1, stops[-1] + 1):
        if live.size:
            q = Q[live]
            for i in range(J):
                t = q[:, idx[i]] - R[i][live]
                a = np.minimum(np.abs(t), 127)
                m1 = a.min(axis=1, keepdims=True)
                rest = a.copy()
                np.put_along_axis(rest, a.argmin(axis=1)[:, None, :], 255, axis=1)
                m2 = rest.min(axis=1, keepdims=True)
                neg = t < 0
                odd = np.logical_xor.reduce(neg, axis=1, keepdims=True) ^ neg      # (the other edges' negative signs)
                mag = (3 * np.where(a == m1, m2, m1)) >> 2
                new = np.where(odd, -mag, mag).astype(np.int16)
                q[:, idx[i]] = t + new
                R[i][live] = new
            Q[live] = q
            iters[live] = it
            bad = np.zeros(live.size, dtype=bool)
            for i in range(J):
                bad |= np.logical_xor.reduce(q[:, idx[i]] < 0, axis=1).any(axis=1)
            conv[live[~bad]] = True
            live = live[bad]
        if it in stops:
            res[it] = ((Q[:, :n] < 0).astype(np.uint8), iters.copy(), conv.copy())
    return res


def ldpc_decode(soft, J, L, max_iter=LDPC_MAX_ITER, perm=None):
    """The integer mirror of ``wofdm_ldpc_decode``, vectorised over the codewords and over the checks of a layer: soft [n_cw, n]
    int8 (d > 0: a coded bit 0), variable c reading soft[:, perm[c]] (None: c); the layered, normalised min-sum decoder of
    include/wofdm.h.  Returns (bits [n_cw, n] uint8, iters [n_cw] int32, converged [n_cw] bool)."""
    return ldpc_decode_at(soft, J, L, (int(max_iter),), perm)[int(max_iter)]


def ldpc_decode_gpu(soft, J, L, max_iter=LDPC_MAX_ITER, perm=None, device=0):
    """``wofdm_ldpc_decode``: soft [n_cw, n] int8 -> (bits [n_cw, n] uint8, iters [n_cw] int32, converged [n_cw] bool).  No CPU
    fallback."""
    from . import _lib
    soft = np.ascontiguousarray(np.atleast_2d(np.asarray(soft)), dtype=np.int8)
    n_cw, n = soft.shape
    p = _check_perm(perm, n)
    bits = np.zeros((n_cw, n), dtype=np.uint8)
    iters, conv = np.zeros(n_cw, dtype=np.int32), np.zeros(n_cw, dtype=np.uint8)
    _lib.check(_lib.load().wofdm_ldpc_decode(int(device), int(J), int(L), int(max_iter), n, None if p is None else p.ctypes.data, n_cw,
                                             soft.ctypes.data, bits.ctypes.data, iters.ctypes.data, conv.ctypes.data))
    return bits, iters, conv != 0


def _ldpc_code_list(codes):
    from . import _lib
    out = []
    for c in ((4, 8),) if codes is None else codes:
        c = tuple(int(x) for x in c)
        if len(c) not in (2, 3):
            raise ValueError("a code is (J, L) or (J, L, max_iter)")
        c = c if len(c) == 3 else c + (LDPC_MAX_ITER,)
        if not (3 <= c[0] <= 6 and c[0] < c[1] <= 24 and 1 <= c[2] <= 64):
            raise ValueError("a code needs 3 <= J <= 6, J < L <= 24 and 1 <= max_iter <= 64")
        out.append(c)
    if not 1 <= len(out) <= _lib.CODE_MAX:
        raise ValueError("1 to %d codes are needed" % _lib.CODE_MAX)
    return out


def ldpc_frame_words(n_f):
    """(W, n): the codewords a frame of n_f coded-stream positions carries and their length, W = ceil(n_f / 16384), n = n_f // W"""
    from . import _lib
    W = -(-int(n_f) // _lib.LDPC_MAX_BITS)
    return W, (int(n_f) // W if W else 0)


def _ldpc_prepare(st, bits_per_sc, syms, act, pil, tps, codes, perm, llr_scale, sym_rot):
    """(codes, perm or None, pos [n_c] as ``_code_prepare``'s, sym_rot, W [points], n [points], K [points, codes])"""
    cl = _ldpc_code_list(codes)
    on = np.ones(st.n_fft, dtype=bool) if act is None else np.asarray(act).reshape(-1) != 0
    data = on & ~pil if pil is not None else on
    pos = (8 * np.flatnonzero(data)[:, None] + np.arange(int(bits_per_sc))[None, :]).reshape(-1)
    if not (np.isfinite(llr_scale) and llr_scale > 0):
        raise ValueError("llr_scale must be finite and positive")
    rot = default_sym_rot(pos.size, max(int(syms) - 1, 1)) % pos.size if sym_rot is None else int(sym_rot)
    if not 0 <= rot < pos.size:
        raise ValueError("sym_rot must be in [0, %d)" % pos.size)
    words = [ldpc_frame_words(pos.size * max(int(syms) - 1 - int(q.post), 0)) for q in tps]
    K = np.array([[n - J * ldpc_lift(J, L, n) if W else 0 for J, L, _ in cl] for W, n in words], dtype=np.int64).reshape(len(tps), len(cl))
    return (cl, _check_perm(perm, pos.size), pos, rot, np.array([w[0] for w in words], dtype=np.int64),
            np.array([w[1] for w in words], dtype=np.int64), K)


def _decode_frame_ldpc(d, tp, pos, perm, codes, sym_rot):
    """{info errors, codeword errors, unconverged, iterations} [codes, 4] of a frame's soft bits d [S - 1, N, 8]: its W codewords"""
    out = np.zeros((len(codes), 4), dtype=np.uint64)
    if d.shape[0] - int(bool(tp.post)) < 1:
        return out
    stream = frame_codewords(d, tp.post, pos, perm, sym_rot)
    W, n = ldpc_frame_words(stream.size)
    words = stream[:W * n].reshape(W, n)
    for i, (J, L, max_iter) in enumerate(codes):
        bits, iters, conv = ldpc_decode(words, J, L, max_iter)
        info = bits[:, J * ldpc_lift(J, L, n):]
        out[i] = info.sum(), info.any(axis=1).sum(), (~conv).sum(), iters.sum()
    return out


def frame_profile_ldpc(st, grids, noise_at, w_tx, w_rx, h, point, tracking, snr_db, bits_per_sc, walk, pilots=None, scales=None,
                       llr_scale=LLR_SCALE, perm=None, codes=None, sym_rot=None, track=None, knot_step=None, ref_power=None,
                       aci_grids=None, aci_h=None, active=None, mask=None, noise_before_truncate=1):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_ldpc``: ``frame_profile_coded``'s outputs through the
    near rule's weight, then {info errors, codeword errors, unconverged, iterations} [codes, 4] of the frame's codewords
    (``ldpc_decode``)."""
    sc = _soft_scales(scales)
    syms = np.asarray(grids).shape[0]
    tps, pil = _tracking_prepare(st, syms, 1, [tracking], pilots, active)
    cl, p, pos, rot = _ldpc_prepare(st, bits_per_sc, syms, active, pil, tps, codes, perm, llr_scale, sym_rot)[:4]
    front, out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power,
                             aci_grids, aci_h, active, mask, noise_before_truncate)
    res = _tracking_outputs(st, front, out, w_rx, snr_db, bits_per_sc, sc, noise_before_truncate, pil, tps[0])
    z, weight = _coded_z(st, front, res, w_rx, snr_db, bits_per_sc, noise_before_truncate, pil, tps[0])
    d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
    d8[..., :z.shape[-1]], t = soft_bits(z, llr_scale)
    return res + (d8, t, weight, _decode_frame_ldpc(d8, tps[0], pos, p, cl, rot))


def _ldpc_result(trk, lerr, K, W, frames, codes, llr_scale, sym_rot, soft):
    return RxProfileLdpc(*trk, *(np.ascontiguousarray(lerr[..., i]) for i in range(4)), K, (W * int(frames)).astype(np.uint64),
                         tuple(codes), float(llr_scale), int(sym_rot), soft)


def rx_profile_ldpc_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                         tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, sym_rot=None,
                         tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                         noise_before_truncate=1, with_near=False, with_soft=False):
    """The host route of ``rx_profile_ldpc_gpu``: ``rx_profile_coded_frame_host``'s frames, points, arrays and soft bits, each
    (frame, point)'s codewords through ``frame_interleaver`` and ``ldpc_decode`` for the codes ``codes`` -- (J, L) or (J, L,
    max_iter) each, None: (4, 8) --; sym_rot None: ``default_sym_rot`` over S - 1 symbols.  Returns ``RxProfileLdpc`` (with_near:
    and the near decisions); with_soft as in ``rx_profile_coded_host``."""
    held = {}

    def receiver(q, n_points, sc):
        tps, pil = _tracking_prepare(st, q.S, n_points, tracking, pilots, q.act)
        cl, p, pos, rot, W, _, K = _ldpc_prepare(st, q.k, q.S, q.act, pil, tps, codes, perm, llr_scale, sym_rot)
        shape = (n_points, q.w_tx.shape[0], q.snr.size, q.hc.shape[0], len(cl), 4)
        held.update(tps=tps, pil=pil, act=q.act, codes=cl, K=K, W=W, rot=rot, lerr=np.zeros(shape, np.uint64))
        if with_soft:
            lead = shape[1:4] + (int(frames), n_points, q.S - 1, st.n_fft)
            held.update(d=np.zeros(lead + (8,), np.int8), t=np.zeros(lead + (q.k,), np.float64), w=np.zeros(lead, np.float64))

        def one(i, tp):
            def run(front, out, p_, s_, c_, f_):
                res = _tracking_outputs(st, front, out, q.w_rx[p_], q.snr[s_], q.k, sc, q.nbt, pil, tp)
                z, weight = _coded_z(st, front, res, q.w_rx[p_], q.snr[s_], q.k, q.nbt, pil, tp)
                d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
                d8[..., :q.k], t = soft_bits(z, llr_scale)
                held["lerr"][i, p_, s_, c_] += _decode_frame_ldpc(d8, tp, pos, p, cl, rot)
                if with_soft:
                    held["d"][p_, s_, c_, f_, i], held["t"][p_, s_, c_, f_, i], held["w"][p_, s_, c_, f_, i] = d8, t, weight
                return res
            return run
        return [one(i, tp) for i, tp in enumerate(tps)]
    res = _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                      knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver)
    soft = res[0] if with_near else res
    dec, sym = _tracking_decisions(st, syms, frames, held["act"], held["pil"], held["tps"])
    trk = RxProfileTracking(*soft[:-1], sym, dec)
    prof = _ldpc_result(trk, held["lerr"], held["K"], held["W"], frames, held["codes"], llr_scale, held["rot"], held.get("d"))
    if with_soft:
        prof = (prof, held["t"], held["w"])
    return (prof, res[1]) if with_near else prof


def rx_profile_ldpc_chunk_frames(st, syms, masked, n_points, neighbour, n_scales):
    """Frames one chunk of ``wofdm_rx_profile_ldpc`` holds: ``rx_profile_coded_chunk_frames``' -- the decoder's state is in LDS"""
    return rx_profile_coded_chunk_frames(st, syms, masked, n_points, neighbour, n_scales)


def rx_profile_ldpc_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                        tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, sym_rot=None,
                        tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                        noise_before_truncate=1, device=0, out=None, export=False):
    """``wofdm_rx_profile_ldpc``: ``rx_profile_coded_frame_gpu``'s frames, tracking fields, soft bits and frame interleaver -- those
    calls' bytes --, and per point and frame W codewords of the quasi-cyclic LDPC codes ``codes`` ((J, L) or (J, L, max_iter)
    each, None: (4, 8)), decoded on the GPU by the layered min-sum decoder.  export=True also returns the soft bits.  Returns
    ``RxProfileLdpc``; ``out`` (an earlier result of the same shape, scales, codes and sym_rot) is accumulated into (its soft bits
    are dropped).  No CPU fallback."""
    import ctypes as C
    from . import _lib
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    tps, pil = _tracking_prepare(st, syms, len(pts), tracking, pilots, prepared[4])
    cl, p, _, rot, W, _, K = _ldpc_prepare(st, bits_per_sc, syms, prepared[4], pil, tps, codes, perm, llr_scale, sym_rot)
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    ctps = (_lib.TrackingPoint * len(tps))(*[_lib.TrackingPoint(q.cpe, q.post, (C.c_int32 * 2)(0, 0)) for q in tps])
    ccodes = (_lib.LdpcCode * len(cl))(*[_lib.LdpcCode(J, L, m, 0) for J, L, m in cl])
    pil8 = None if pil is None else np.ascontiguousarray(pil, dtype=np.uint8)
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if not np.array_equal(out.scales, sc) or tuple(out.codes) != tuple(cl) or out.sym_rot != rot:
            raise ValueError("out has other scales, codes or sym_rot")
        prev = _RxSoftSums(*out[:9], np.zeros(st.n_fft, dtype=np.uint64))
    cells = (prepared[0].shape[0], prepared[3].size, prepared[2].shape[0])
    lerr = np.zeros((len(pts),) + cells + (len(cl), 4), dtype=np.uint64)
    sb = np.zeros(cells + (int(frames), len(pts), int(syms) - 1, st.n_fft, 8), dtype=np.int8) if export else None
    res = _gpu_call("wofdm_rx_profile_ldpc", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data, None if pil8 is None else pil8.ctypes.data, ctps,
                                C.c_float(float(llr_scale)), None if p is None else p.ctypes.data, len(cl), ccodes, int(rot)),
                    behind=(lerr.ctypes.data, None if sb is None else sb.ctypes.data))
    dec, sym = _tracking_decisions(st, syms, frames, prepared[4], pil, tps)
    if out is not None:
        if out.decisions.shape != dec.shape:
            raise ValueError("out has another shape")
        dec, sym = out.decisions + dec, out.decisions_sym + sym
    prof = _ldpc_result(_tracking_result(res, sc, dec, sym), lerr, K, W, frames, cl, llr_scale, rot, sb)
    if out is not None:
        prof = prof._replace(info_err=out.info_err + prof.info_err, cw_err=out.cw_err + prof.cw_err,
                             unconverged=out.unconverged + prof.unconverged, iterations=out.iterations + prof.iterations,
                             codewords=out.codewords + prof.codewords)
    return prof


def _ldpc_per_word(prof, counts, per_word):
    words = (prof.codewords.astype(np.float64)[:, None] * per_word).reshape(
        (counts.shape[0],) + (1,) * (counts.ndim - 2) + (-1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(words > 0, counts.astype(np.float64) / np.where(words > 0, words, 1.0), np.nan)


def ldpc_ber(prof):
    """The decoded info-bit error rate of the frames' codewords [points, pairs, n_snr, n_ch, codes]; NaN where a point carried no
    codeword"""
    return _ldpc_per_word(prof, prof.info_err, prof.info_bits.astype(np.float64))


def ldpc_fer(prof):
    """The codeword error rate (any info bit wrong), shaped as ``ldpc_ber``'s"""
    return _ldpc_per_word(prof, prof.cw_err, (prof.info_bits > 0).astype(np.float64))


def ldpc_mean_iterations(prof):
    """The iterations run per codeword, shaped as ``ldpc_ber``'s"""
    return _ldpc_per_word(prof, prof.iterations, (prof.info_bits > 0).astype(np.float64))


# ---- random information words: both decoders in the coset view (wofdm_rx_profile_coset), the encoders on the GPU ----

#: the Philox stream of the information words (csrc/wofdm_link.h), beside ``STREAM_BITS`` ... ``STREAM_PN``
STREAM_INFO = 4

RxProfileCoset = collections.namedtuple(
    "RxProfileCoset", RxProfileTracking._fields + (
        "info_err", "cw_err", "info_bits", "codewords", "rates",
        "ldpc_info_err", "ldpc_cw_err", "unconverged", "iterations", "ldpc_info_bits", "ldpc_codewords", "ldpc_codes",
        "llr_scale", "sym_rot", "soft_bits"))
RxProfileCoset.__doc__ = """``RxProfileTracking``'s fields; info_err, cw_err, info_bits, codewords, rates as ``RxProfileCodedFrame``'s
and ldpc_info_err, ldpc_cw_err, unconverged, iterations, ldpc_info_bits, ldpc_codewords, ldpc_codes as ``RxProfileLdpc``'s info_err
... codes -- but against RANDOM transmitted words, the frame's information stream encoded (``coset_codewords``), where those count
against the all-zero word; a family without a code has arrays with a code axis of length 0; llr_scale; sym_rot; soft_bits as
theirs."""


def coset_info(seed, cell, frame, n_bits):
    """Bits 0 ... n_bits - 1 (uint8) of the information stream of (seed, cell, frame), ``wofdm_coset_info``: Philox stream 4,
    bit i is bit i mod 32 of word (i mod 128) div 32 of block i div 128"""
    n_bits = int(n_bits)
    w = _stream(seed, STREAM_INFO, cell, frame, max((n_bits + 127) // 128, 1)).reshape(-1)
    i = np.arange(n_bits, dtype=np.int64)
    return ((w[i >> 5] >> (i & 31).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def conv_encode_gpu(info, rate, n_c, device=0):
    """``wofdm_conv_encode``: info [n_cw, T - 6] bits, T = ``code_steps``(rate, n_c) -> the coded stream [n_cw, n_c] (uint8):
    ``conv_encode``'s kept outputs, zeros on the left-over positions.  No CPU fallback."""
    from . import _lib
    info = np.ascontiguousarray(np.atleast_2d(np.asarray(info)), dtype=np.uint8)
    steps = code_steps(rate, n_c)
    if info.shape[1] != steps - 6:
        raise ValueError("a word has T - 6 = %d information bits" % (steps - 6))
    coded = np.zeros((info.shape[0], int(n_c)), dtype=np.uint8)
    _lib.check(_lib.load().wofdm_conv_encode(int(device), int(rate), int(n_c), info.shape[0], info.ctypes.data, coded.ctypes.data))
    return coded


def ldpc_encode_gpu(info, J, L, n, device=0):
    """``wofdm_ldpc_encode``: info [n_cw, K] bits -> the codewords [n_cw, n] (uint8), ``ldpc_encode``'s.  No CPU fallback."""
    from . import _lib
    info = np.ascontiguousarray(np.atleast_2d(np.asarray(info)), dtype=np.uint8)
    K = int(n) - int(J) * ldpc_lift(J, L, n)
    if info.shape[1] != K:
        raise ValueError("the code has K = %d information bits" % K)
    word = np.zeros((info.shape[0], int(n)), dtype=np.uint8)
    _lib.check(_lib.load().wofdm_ldpc_encode(int(device), int(J), int(L), int(n), info.shape[0], info.ctypes.data, word.ctypes.data))
    return word


def _coset_lists(codes, ldpc_codes):
    """(rates, LDPC codes): ``_code_list`` and ``_ldpc_code_list``, either of which an empty sequence switches off"""
    rates = [] if codes is not None and len(codes) == 0 else _code_list(codes)
    cl = [] if ldpc_codes is not None and len(ldpc_codes) == 0 else _ldpc_code_list(ldpc_codes)
    if not rates and not cl:
        raise ValueError("at least one code is needed")
    return rates, cl


def coset_codewords(seed, cell, frame, n_f, codes=None, ldpc_codes=None):
    """The transmitted coded streams of one (cell, frame) whose frame has n_f coded-stream positions, as
    ``wofdm_rx_profile_coset`` forms them -- for a decoder of the caller's own: (x [codes, n_f], x_ldpc [ldpc codes, n_f]), uint8.
    A Viterbi code's word is ``conv_encode`` of stream bits 0 ... T - 7; LDPC word w of a code, at coded-stream indices w n ... w n
    + n - 1, is ``ldpc_encode`` of stream bits w n ... w n + K - 1; left-over positions are 0.  A soft bit d of coded-stream index
    c (``frame_codewords``) reaches the decoder as -d where x[c] is 1."""
    rates, cl = _coset_lists(codes, ldpc_codes)
    n_f = int(n_f)
    stream = coset_info(seed, cell, frame, n_f)
    xv, xl = np.zeros((len(rates), n_f), dtype=np.uint8), np.zeros((len(cl), n_f), dtype=np.uint8)
    for i, r in enumerate(rates):
        word = conv_encode(stream[:code_steps(r, n_f) - 6], r)
        xv[i, :word.size] = word
    W, n = ldpc_frame_words(n_f)
    for i, (J, L, _) in enumerate(cl):
        K = n - J * ldpc_lift(J, L, n)
        info = np.stack([stream[w * n:w * n + K] for w in range(W)])
        xl[i, :W * n] = ldpc_encode(info, J, L, n).reshape(-1)
    return xv, xl


def _coset_prepare(st, bits_per_sc, syms, act, pil, tps, codes, ldpc_codes, perm, llr_scale, sym_rot):
    """(rates, LDPC codes, perm or None, pos, sym_rot, T [points, codes], W [points], K [points, ldpc codes]): ``_frame_code_prepare``
    and ``_ldpc_prepare`` for the families in use"""
    rates, cl = _coset_lists(codes, ldpc_codes)
    steps = np.zeros((len(tps), 0), dtype=np.int64)
    W, K = np.zeros(len(tps), dtype=np.int64), np.zeros((len(tps), 0), dtype=np.int64)
    if rates:
        _, p, pos, rot, steps = _frame_code_prepare(st, bits_per_sc, syms, act, pil, tps, rates, perm, llr_scale, sym_rot)
    if cl:
        _, p, pos, rot, W, _, K = _ldpc_prepare(st, bits_per_sc, syms, act, pil, tps, cl, perm, llr_scale, sym_rot)
    return rates, cl, p, pos, rot, steps, W, K


def _decode_frame_coset(d, tp, pos, perm, rates, cl, sym_rot, seed, cell, frame):
    """({info errors, codeword errors} [codes, 2], {info errors, codeword errors, unconverged, iterations} [ldpc codes, 4]) of a
    frame's soft bits d [S - 1, N, 8] against the transmitted words of (seed, cell, frame): the mirror decoders on d' = x ? -d : d"""
    ferr, lerr = np.zeros((len(rates), 2), dtype=np.uint64), np.zeros((len(cl), 4), dtype=np.uint64)
    if d.shape[0] - int(bool(tp.post)) < 1:
        return ferr, lerr
    soft = frame_codewords(d, tp.post, pos, perm, sym_rot).astype(np.int16)
    xv, xl = coset_codewords(seed, cell, frame, soft.size, rates, cl)
    for i, r in enumerate(rates):
        bits, _ = viterbi_decode(np.where(xv[i] != 0, -soft, soft)[None], r)
        T = bits.shape[1]
        wrong = bits[0] ^ np.concatenate([coset_info(seed, cell, frame, T - 6), np.zeros(6, np.uint8)])
        ferr[i] = wrong[:T - 6].sum(), wrong.any()
    W, n = ldpc_frame_words(soft.size)
    for i, (J, L, max_iter) in enumerate(cl):
        bits, iters, conv = ldpc_decode(np.where(xl[i] != 0, -soft, soft)[:W * n].reshape(W, n), J, L, max_iter)
        wrong = (bits ^ xl[i, :W * n].reshape(W, n))[:, J * ldpc_lift(J, L, n):]
        lerr[i] = wrong.sum(), wrong.any(axis=1).sum(), (~conv).sum(), iters.sum()
    return ferr, lerr


def frame_profile_coset(st, grids, noise_at, w_tx, w_rx, h, point, tracking, snr_db, bits_per_sc, walk, seed, cell, frame, pilots=None,
                        scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, ldpc_codes=None, sym_rot=None, track=None,
                        knot_step=None, ref_power=None, aci_grids=None, aci_h=None, active=None, mask=None, noise_before_truncate=1):
    """fp64 host mirror of one frame and one point of ``wofdm_rx_profile_coset``: ``frame_profile_coded``'s outputs through the near
    rule's weight, then ``_decode_frame_coset``'s two arrays -- the frame's words are those of the information stream of (seed, cell,
    frame), which the caller names beside the randomness it hands in."""
    sc = _soft_scales(scales)
    syms = np.asarray(grids).shape[0]
    tps, pil = _tracking_prepare(st, syms, 1, [tracking], pilots, active)
    rates, cl, p, pos, rot = _coset_prepare(st, bits_per_sc, syms, active, pil, tps, codes, ldpc_codes, perm, llr_scale, sym_rot)[:5]
    front, out = _frame_link(st, grids, noise_at, w_tx, w_rx, h, point, snr_db, bits_per_sc, walk, track, knot_step, ref_power,
                             aci_grids, aci_h, active, mask, noise_before_truncate)
    res = _tracking_outputs(st, front, out, w_rx, snr_db, bits_per_sc, sc, noise_before_truncate, pil, tps[0])
    z, weight = _coded_z(st, front, res, w_rx, snr_db, bits_per_sc, noise_before_truncate, pil, tps[0])
    d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
    d8[..., :z.shape[-1]], t = soft_bits(z, llr_scale)
    return res + (d8, t, weight) + _decode_frame_coset(d8, tps[0], pos, p, rates, cl, rot, seed, cell, frame)


def _coset_result(trk, ferr, lerr, steps, W, K, frames, rates, cl, llr_scale, sym_rot, soft):
    words = np.full(steps.shape[0], int(frames), dtype=np.uint64)
    return RxProfileCoset(*trk, np.ascontiguousarray(ferr[..., 0]), np.ascontiguousarray(ferr[..., 1]), np.maximum(steps - 6, 0), words,
                          tuple(rates), *(np.ascontiguousarray(lerr[..., i]) for i in range(4)), K, (W * int(frames)).astype(np.uint64),
                          tuple(cl), float(llr_scale), int(sym_rot), soft)


def rx_profile_coset_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                          tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, ldpc_codes=None,
                          sym_rot=None, tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                          noise_before_truncate=1, with_near=False, with_soft=False):
    """The host route of ``rx_profile_coset_gpu``: ``rx_profile_coded_frame_host``'s frames, points, arrays and soft bits, each
    (frame, point)'s words drawn, encoded and decoded by the mirrors (``_decode_frame_coset``).  Returns ``RxProfileCoset``
    (with_near: and the near decisions); with_soft as in ``rx_profile_coded_host``."""
    held = {}

    def receiver(q, n_points, sc):
        tps, pil = _tracking_prepare(st, q.S, n_points, tracking, pilots, q.act)
        rates, cl, p, pos, rot, steps, W, K = _coset_prepare(st, q.k, q.S, q.act, pil, tps, codes, ldpc_codes, perm, llr_scale, sym_rot)
        shape = (n_points, q.w_tx.shape[0], q.snr.size, q.hc.shape[0])
        held.update(tps=tps, pil=pil, act=q.act, rates=rates, cl=cl, steps=steps, W=W, K=K, rot=rot,
                    ferr=np.zeros(shape + (len(rates), 2), np.uint64), lerr=np.zeros(shape + (len(cl), 4), np.uint64))
        if with_soft:
            lead = shape[1:4] + (int(frames), n_points, q.S - 1, st.n_fft)
            held.update(d=np.zeros(lead + (8,), np.int8), t=np.zeros(lead + (q.k,), np.float64), w=np.zeros(lead, np.float64))

        def one(i, tp):
            def run(front, out, p_, s_, c_, f_):
                res = _tracking_outputs(st, front, out, q.w_rx[p_], q.snr[s_], q.k, sc, q.nbt, pil, tp)
                z, weight = _coded_z(st, front, res, q.w_rx[p_], q.snr[s_], q.k, q.nbt, pil, tp)
                d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
                d8[..., :q.k], t = soft_bits(z, llr_scale)
                cell = (p_ * q.snr.size + s_) * q.hc.shape[0] + c_
                ferr, lerr = _decode_frame_coset(d8, tp, pos, p, rates, cl, rot, seed, cell, int(frame_offset) + f_)
                held["ferr"][i, p_, s_, c_] += ferr
                held["lerr"][i, p_, s_, c_] += lerr
                if with_soft:
                    held["d"][p_, s_, c_, f_, i], held["t"][p_, s_, c_, f_, i], held["w"][p_, s_, c_, f_, i] = d8, t, weight
                return res
            return run
        return [one(i, tp) for i, tp in enumerate(tps)]
    res = _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                      knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver)
    soft = res[0] if with_near else res
    dec, sym = _tracking_decisions(st, syms, frames, held["act"], held["pil"], held["tps"])
    trk = RxProfileTracking(*soft[:-1], sym, dec)
    prof = _coset_result(trk, held["ferr"], held["lerr"], held["steps"], held["W"], held["K"], frames, held["rates"], held["cl"],
                         llr_scale, held["rot"], held.get("d"))
    if with_soft:
        prof = (prof, held["t"], held["w"])
    return (prof, res[1]) if with_near else prof


def rx_profile_coset_chunk_frames(st, bits_per_sc, syms, masked, n_points, neighbour, n_scales, n_data_bins, codes=(0,), post=False):
    """Frames one chunk of ``wofdm_rx_profile_coset`` holds: ``rx_profile_coded_frame_chunk_frames``' with the Viterbi rates
    ``codes``, and without any (an empty sequence) ``rx_profile_ldpc_chunk_frames``' -- the history term only where a Viterbi code
    runs"""
    if len(codes) == 0:
        return rx_profile_ldpc_chunk_frames(st, syms, masked, n_points, neighbour, n_scales)
    return rx_profile_coded_frame_chunk_frames(st, bits_per_sc, syms, masked, n_points, neighbour, n_scales, n_data_bins, codes, post)


def rx_profile_coset_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                         tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, codes=None, ldpc_codes=None,
                         sym_rot=None, tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None, mask=None,
                         noise_before_truncate=1, device=0, out=None, export=False):
    """``wofdm_rx_profile_coset``: ``rx_profile_coded_frame_gpu``'s and ``rx_profile_ldpc_gpu``'s frames, tracking fields, soft bits
    and frame interleaver -- those calls' bytes --, both decoders behind ONE receive chain, and random transmitted words in the
    place of the all-zero one: the frame's information stream (``coset_info``) encoded on the GPU inside the decoders.  ``codes``
    are Viterbi rates (None: rate 1/2; an empty sequence: none), ``ldpc_codes`` (J, L) or (J, L, max_iter) each (None: (4, 8); an
    empty sequence: none).  export=True also returns the soft bits.  Returns ``RxProfileCoset``; ``out`` (an earlier result of the
    same shape, scales, codes and sym_rot) is accumulated into (its soft bits are dropped).  No CPU fallback."""
    import ctypes as C
    from . import _lib
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    tps, pil = _tracking_prepare(st, syms, len(pts), tracking, pilots, prepared[4])
    rates, cl, p, _, rot, steps, W, K = _coset_prepare(st, bits_per_sc, syms, prepared[4], pil, tps, codes, ldpc_codes, perm, llr_scale,
                                                       sym_rot)
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    ctps = (_lib.TrackingPoint * len(tps))(*[_lib.TrackingPoint(q.cpe, q.post, (C.c_int32 * 2)(0, 0)) for q in tps])
    ccodes = (_lib.Code * max(len(rates), 1))(*[_lib.Code(r, (C.c_int32 * 3)(0, 0, 0)) for r in rates])
    lcodes = (_lib.LdpcCode * max(len(cl), 1))(*[_lib.LdpcCode(J, L, m, 0) for J, L, m in cl])
    pil8 = None if pil is None else np.ascontiguousarray(pil, dtype=np.uint8)
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if (not np.array_equal(out.scales, sc) or tuple(out.rates) != tuple(rates) or tuple(out.ldpc_codes) != tuple(cl)
                or out.sym_rot != rot):
            raise ValueError("out has other scales, codes or sym_rot")
        prev = _RxSoftSums(*out[:9], np.zeros(st.n_fft, dtype=np.uint64))
    cells = (prepared[0].shape[0], prepared[3].size, prepared[2].shape[0])
    ferr = np.zeros((len(pts),) + cells + (len(rates), 2), dtype=np.uint64)
    lerr = np.zeros((len(pts),) + cells + (len(cl), 4), dtype=np.uint64)
    sb = np.zeros(cells + (int(frames), len(pts), int(syms) - 1, st.n_fft, 8), dtype=np.int8) if export else None
    res = _gpu_call("wofdm_rx_profile_coset", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data, None if pil8 is None else pil8.ctypes.data, ctps,
                                C.c_float(float(llr_scale)), None if p is None else p.ctypes.data, len(rates), ccodes if rates else None,
                                len(cl), lcodes if cl else None, int(rot)),
                    behind=(ferr.ctypes.data if rates else None, lerr.ctypes.data if cl else None,
                            None if sb is None else sb.ctypes.data))
    dec, sym = _tracking_decisions(st, syms, frames, prepared[4], pil, tps)
    if out is not None:
        if out.decisions.shape != dec.shape:
            raise ValueError("out has another shape")
        dec, sym = out.decisions + dec, out.decisions_sym + sym
    prof = _coset_result(_tracking_result(res, sc, dec, sym), ferr, lerr, steps, W, K, frames, rates, cl, llr_scale, rot, sb)
    if out is not None:
        prof = prof._replace(**{f: getattr(out, f) + getattr(prof, f) for f in (
            "info_err", "cw_err", "codewords", "ldpc_info_err", "ldpc_cw_err", "unconverged", "iterations", "ldpc_codewords")})
    return prof


def _coset_views(prof):
    """``prof`` as an ``RxProfileCodedFrame`` and an ``RxProfileLdpc``, for their rate functions"""
    n = len(RxProfileTracking._fields)
    return (RxProfileCodedFrame(*prof[:n], prof.info_err, prof.cw_err, prof.info_bits, prof.codewords, prof.rates, prof.llr_scale,
                                prof.sym_rot, None),
            RxProfileLdpc(*prof[:n], prof.ldpc_info_err, prof.ldpc_cw_err, prof.unconverged, prof.iterations, prof.ldpc_info_bits,
                          prof.ldpc_codewords, prof.ldpc_codes, prof.llr_scale, prof.sym_rot, None))


def coset_ber(prof):
    """(Viterbi, LDPC): the decoded info-bit error rates against the transmitted words, [points, pairs, n_snr, n_ch, codes] each, as
    ``coded_frame_ber`` and ``ldpc_ber`` form them"""
    vit, ldpc = _coset_views(prof)
    return coded_frame_ber(vit), ldpc_ber(ldpc)


def coset_fer(prof):
    """(Viterbi, LDPC): the codeword error rates, as ``coded_fer`` and ``ldpc_fer`` form them"""
    vit, ldpc = _coset_views(prof)
    return coded_fer(vit), ldpc_fer(ldpc)


# ---- retransmissions with soft combining (wofdm_rx_profile_harq, wofdm_ldpc_harq_decode) ----

RxProfileHarq = collections.namedtuple(
    "RxProfileHarq", RxProfileTracking._fields + (
        "acked", "unacked", "word_err", "undetected", "info_err", "iterations", "info_bits", "word_bits", "frame_words", "words",
        "codes", "rounds", "combine", "llr_scale", "sym_rot", "soft_bits"))
RxProfileHarq.__doc__ = """``RxProfileTracking``'s fields, and the counters of include/wofdm.h's HARQ block (uint64): acked [points,
pairs, n_snr, n_ch, codes, 8]: the words ACKed at round 1 ... 8; unacked, word_err, undetected, info_err, iterations [points, pairs,
n_snr, n_ch, codes]: the words never ACKed, those with a wrong information bit at the stop, of those the ACKed ones, the
information-bit errors at the stop and the iterations over all rounds; info_bits [points, codes]: K; word_bits [points]: n;
frame_words [points]: W, the words of a frame; words [points]: the words per cell, W times the groups; codes [codes]: (J, L,
max_iter); rounds; combine; llr_scale; sym_rot; soft_bits as ``RxProfileCoset``'s."""


def _harq_args(rounds, combine):
    from . import _lib
    rounds, combine = int(rounds), int(bool(combine)) if isinstance(combine, (bool, np.bool_)) else int(combine)
    if not 1 <= rounds <= _lib.HARQ_MAX_ROUNDS:
        raise ValueError("rounds must be 1 ... %d" % _lib.HARQ_MAX_ROUNDS)
    if combine not in (0, 1):
        raise ValueError("combine must be 0 or 1")
    return rounds, combine


def ldpc_harq_decode(soft, J, L, max_iter=LDPC_MAX_ITER, combine=True, perm=None):
    """The integer mirror of ``wofdm_ldpc_harq_decode``, built on ``ldpc_decode``: soft [n_cw, rounds, n] int8, the transmissions
    d' of each word.  Round r decodes q = clip(sum of rows 0 ... r, -127, 127) (combine) or clip(row r, -127, 127), formed in
    int32, afresh; the first round that converges ends the word, a word that never does stops after the last round with that
    round's decisions.  Returns (bits [n_cw, n] uint8, round [n_cw] int32 the 1-based stop round, iters [n_cw] int32 over all
    rounds, converged [n_cw] bool)."""
    d = np.asarray(soft)
    d = (d[None] if d.ndim == 2 else d).astype(np.int32)
    n_cw, rounds, n = d.shape
    rounds, combine = _harq_args(rounds, combine)
    bits = np.zeros((n_cw, n), dtype=np.uint8)
    rnd, iters, conv = np.full(n_cw, rounds, dtype=np.int32), np.zeros(n_cw, dtype=np.int32), np.zeros(n_cw, dtype=bool)
    live = np.arange(n_cw)
    for r in range(rounds):
        if not live.size:
            break
        q = np.clip(d[live, :r + 1].sum(axis=1) if combine else d[live, r], -127, 127).astype(np.int16)
        b, it, cv = ldpc_decode(q, J, L, max_iter, perm)
        bits[live], conv[live] = b, cv
        iters[live] += it
        rnd[live[cv]] = r + 1
        live = live[~cv]
    return bits, rnd, iters, conv


def ldpc_harq_decode_gpu(soft, J, L, max_iter=LDPC_MAX_ITER, combine=True, perm=None, device=0):
    """``wofdm_ldpc_harq_decode``: soft [n_cw, rounds, n] int8 -> (bits [n_cw, n] uint8, round [n_cw] int32, iters [n_cw] int32,
    converged [n_cw] bool), ``ldpc_harq_decode``'s.  No CPU fallback."""
    from . import _lib
    soft = np.asarray(soft)
    soft = np.ascontiguousarray(soft[None] if soft.ndim == 2 else soft, dtype=np.int8)
    n_cw, rounds, n = soft.shape
    p = _check_perm(perm, n)
    bits = np.zeros((n_cw, n), dtype=np.uint8)
    rnd, iters, conv = np.zeros(n_cw, dtype=np.int32), np.zeros(n_cw, dtype=np.int32), np.zeros(n_cw, dtype=np.uint8)
    _lib.check(_lib.load().wofdm_ldpc_harq_decode(int(device), int(J), int(L), int(max_iter), n, None if p is None else p.ctypes.data,
                                                  n_cw, rounds, int(combine), soft.ctypes.data, bits.ctypes.data, rnd.ctypes.data,
                                                  iters.ctypes.data, conv.ctypes.data))
    return bits, rnd, iters, conv != 0


def _harq_prepare(rounds, combine, frame_offset, frames):
    rounds, combine = _harq_args(rounds, combine)
    if int(frames) % rounds or int(frame_offset) % rounds:
        raise ValueError("frames and frame_offset must be multiples of rounds")
    return rounds, combine


def _decode_group_harq(rows, cl, combine, seed, cell, frame0):
    """The counters [codes, 13] of one group and point: rows [rounds, n_f] the frames' coded streams (``frame_codewords``), the
    words those of the information stream of (seed, cell, frame0), the group's first frame"""
    from . import _lib
    rows = np.asarray(rows).astype(np.int16)
    out = np.zeros((len(cl), _lib.HARQ_FIELDS), dtype=np.uint64)
    xl = coset_codewords(seed, cell, frame0, rows.shape[1], (), cl)[1]
    W, n = ldpc_frame_words(rows.shape[1])
    for i, (J, L, max_iter) in enumerate(cl):
        d = np.where(xl[i] != 0, -rows, rows)[:, :W * n].reshape(rows.shape[0], W, n).transpose(1, 0, 2)
        bits, rnd, iters, conv = ldpc_harq_decode(d, J, L, max_iter, combine)
        wrong = (bits ^ xl[i, :W * n].reshape(W, n))[:, J * ldpc_lift(J, L, n):]
        bad = wrong.any(axis=1)
        out[i, :8] = np.bincount(rnd[conv] - 1, minlength=8)
        out[i, 8:] = (~conv).sum(), bad.sum(), (bad & conv).sum(), wrong.sum(), iters.sum()
    return out


def _harq_result(trk, herr, K, W, n, frames, cl, rounds, combine, llr_scale, sym_rot, soft):
    f = [np.ascontiguousarray(herr[..., i]) for i in range(8, 13)]
    return RxProfileHarq(*trk, np.ascontiguousarray(herr[..., :8]), *f, K, n, W, (W * (int(frames) // rounds)).astype(np.uint64),
                         tuple(cl), rounds, combine, float(llr_scale), int(sym_rot), soft)


def rx_profile_harq_host(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                         tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, ldpc_codes=None, sym_rot=None,
                         rounds=4, combine=True, tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None,
                         mask=None, noise_before_truncate=1, with_near=False):
    """The host route of ``rx_profile_harq_gpu``, composed of ``rx_profile_coset_host``'s pieces: its frames, points, arrays and
    soft bits; the frames of a cell in groups of ``rounds``, each group's words drawn from its first frame and decoded by
    ``ldpc_harq_decode`` on the frames' coded streams.  Returns ``RxProfileHarq`` (with_near: and the near decisions)."""
    from . import _lib
    rounds, combine = _harq_prepare(rounds, combine, frame_offset, frames)
    held = {}

    def receiver(q, n_points, sc):
        tps, pil = _tracking_prepare(st, q.S, n_points, tracking, pilots, q.act)
        _, cl, p, pos, rot, _, W, K = _coset_prepare(st, q.k, q.S, q.act, pil, tps, (), ldpc_codes, perm, llr_scale, sym_rot)
        n = np.array([ldpc_frame_words(pos.size * max(q.S - 1 - int(t.post), 0))[1] for t in tps], dtype=np.int64)
        shape = (n_points, q.w_tx.shape[0], q.snr.size, q.hc.shape[0])
        held.update(tps=tps, pil=pil, act=q.act, cl=cl, W=W, K=K, n=n, rot=rot, rows={},
                    herr=np.zeros(shape + (len(cl), _lib.HARQ_FIELDS), np.uint64))

        def one(i, tp):
            def run(front, out, p_, s_, c_, f_):
                res = _tracking_outputs(st, front, out, q.w_rx[p_], q.snr[s_], q.k, sc, q.nbt, pil, tp)
                z, _ = _coded_z(st, front, res, q.w_rx[p_], q.snr[s_], q.k, q.nbt, pil, tp)
                d8 = np.zeros(z.shape[:2] + (8,), dtype=np.int8)
                d8[..., :q.k] = soft_bits(z, llr_scale)[0]
                if d8.shape[0] - int(bool(tp.post)) >= 1:
                    rows = held["rows"].setdefault((i, p_, s_, c_, f_ // rounds), {})
                    rows[f_ % rounds] = frame_codewords(d8, tp.post, pos, p, rot)
                    if len(rows) == rounds:
                        cell = (p_ * q.snr.size + s_) * q.hc.shape[0] + c_
                        frame0 = int(frame_offset) + (f_ // rounds) * rounds
                        held["herr"][i, p_, s_, c_] += _decode_group_harq([rows[r] for r in range(rounds)], cl, combine, seed, cell, frame0)
                        del held["rows"][(i, p_, s_, c_, f_ // rounds)]
                return res
            return run
        return [one(i, tp) for i, tp in enumerate(tps)]
    res = _soft_sweep(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points, scales, tracks,
                      knot_step, aci_active, aci_h, ref_power, active, mask, noise_before_truncate, with_near, receiver)
    soft = res[0] if with_near else res
    dec, sym = _tracking_decisions(st, syms, frames, held["act"], held["pil"], held["tps"])
    trk = RxProfileTracking(*soft[:-1], sym, dec)
    prof = _harq_result(trk, held["herr"], held["K"], held["W"], held["n"], frames, held["cl"], rounds, combine, llr_scale, held["rot"],
                        None)
    return (prof, res[1]) if with_near else prof


def rx_profile_harq_chunk_frames(st, syms, masked, n_points, neighbour, n_scales, rounds):
    """Frames one chunk of ``wofdm_rx_profile_harq`` holds: ``rx_profile_ldpc_chunk_frames``' rounded down to a multiple of
    ``rounds``, and ``rounds`` where that would be 0 -- a group never straddles a chunk"""
    rounds = _harq_args(rounds, 1)[0]
    return max(rx_profile_ldpc_chunk_frames(st, syms, masked, n_points, neighbour, n_scales) // rounds, 1) * rounds


def rx_profile_harq_gpu(st, bits_per_sc, syms, w_tx_pairs, w_rx_pairs, h, snr_db, seed, frame_offset, frames, points=None,
                        tracking=None, pilots=None, scales=None, llr_scale=LLR_SCALE, perm=None, ldpc_codes=None, sym_rot=None,
                        rounds=4, combine=True, tracks=None, knot_step=None, aci_active=None, aci_h=None, ref_power=None, active=None,
                        mask=None, noise_before_truncate=1, device=0, out=None, export=False):
    """``wofdm_rx_profile_harq``: ``rx_profile_coset_gpu``'s frames, tracking fields, soft bits and frame interleaver -- those calls'
    bytes --, the frames of a cell in groups of ``rounds`` transmissions of the same LDPC words (``ldpc_codes``: (J, L) or (J, L,
    max_iter) each, None: (4, 8)), combined (``combine``: Chase, or the last transmission alone) and decoded on the GPU until the
    syndrome vanishes.  ``frames`` and ``frame_offset`` must be multiples of ``rounds``.  export=True also returns the soft bits.
    Returns ``RxProfileHarq``; ``out`` (an earlier result of the same shape, scales, codes, rounds, combine and sym_rot) is
    accumulated into (its soft bits are dropped).  No CPU fallback."""
    import ctypes as C
    from . import _lib
    rounds, combine = _harq_prepare(rounds, combine, frame_offset, frames)
    sc = _soft_scales(scales)
    points = [LinkPoint()] if points is None else points
    prepared = _prepare(st, w_tx_pairs, w_rx_pairs, h, snr_db, active, mask)
    pts, tr, iact, hi, ref = _link_sides(st, prepared[2], points, tracks, aci_active, aci_h, ref_power, prepared[0].shape[0])
    tps, pil = _tracking_prepare(st, syms, len(pts), tracking, pilots, prepared[4])
    cl, p, pos, rot, W, n, K = _ldpc_prepare(st, bits_per_sc, syms, prepared[4], pil, tps, ldpc_codes, perm, llr_scale, sym_rot)
    trf = None if tr is None else _lib.c64_as_f32(tr)
    hif = None if hi is None else _lib.c64_as_f32(hi)
    lin = PaPoint(PA_LINEAR, 0.0)
    cpts = (_lib.LinkPoint * len(pts))(*[
        _lib.LinkPoint(*(q.pa or lin), -1 if q.track is None else q.track, q.timing, q.cfo, q.cfo_tracked, q.linewidth, q.cpe_tracked,
                       int(q.aci is not None), *(q.aci or (0, 0.0)), (C.c_int32 * 4)(0, 0, 0, 0)) for q in pts])
    ctps = (_lib.TrackingPoint * len(tps))(*[_lib.TrackingPoint(q.cpe, q.post, (C.c_int32 * 2)(0, 0)) for q in tps])
    lcodes = (_lib.LdpcCode * len(cl))(*[_lib.LdpcCode(J, L, m, 0) for J, L, m in cl])
    pil8 = None if pil is None else np.ascontiguousarray(pil, dtype=np.uint8)
    knots = (0, 0, 0) if tr is None else (tr.shape[0], tr.shape[2], int(knot_step))
    prev = None
    if out is not None:
        if (not np.array_equal(out.scales, sc) or tuple(out.codes) != tuple(cl) or out.sym_rot != rot or out.rounds != rounds
                or out.combine != combine):
            raise ValueError("out has other scales, codes, rounds, combine or sym_rot")
        prev = _RxSoftSums(*out[:9], np.zeros(st.n_fft, dtype=np.uint64))
    cells = (prepared[0].shape[0], prepared[3].size, prepared[2].shape[0])
    herr = np.zeros((len(pts),) + cells + (len(cl), _lib.HARQ_FIELDS), dtype=np.uint64)
    sb = np.zeros(cells + (int(frames), len(pts), int(syms) - 1, st.n_fft, 8), dtype=np.int8) if export else None
    res = _gpu_call("wofdm_rx_profile_harq", _RxSoftSums, st, bits_per_sc, syms, prepared, seed, frame_offset, frames,
                    noise_before_truncate, device, prev, lead=(len(pts),), n_scales=sc.size,
                    after_mask=(None if trf is None else trf.ctypes.data, *knots, None if iact is None else iact.ctypes.data,
                                None if hif is None else hif.ctypes.data, None if ref is None else ref.ctypes.data, len(pts), cpts,
                                int(sc.size), sc.ctypes.data, None if pil8 is None else pil8.ctypes.data, ctps,
                                C.c_float(float(llr_scale)), None if p is None else p.ctypes.data, len(cl), lcodes, int(rot), rounds,
                                combine),
                    behind=(herr.ctypes.data, None if sb is None else sb.ctypes.data))
    dec, sym = _tracking_decisions(st, syms, frames, prepared[4], pil, tps)
    if out is not None:
        if out.decisions.shape != dec.shape:
            raise ValueError("out has another shape")
        dec, sym = out.decisions + dec, out.decisions_sym + sym
    prof = _harq_result(_tracking_result(res, sc, dec, sym), herr, K, W, n, frames, cl, rounds, combine, llr_scale, rot, sb)
    if out is not None:
        prof = prof._replace(**{f: getattr(out, f) + getattr(prof, f) for f in (
            "acked", "unacked", "word_err", "undetected", "info_err", "iterations", "words")})
    return prof


def _harq_words(prof, like):
    """The words per cell of each point and code, shaped to divide ``like`` [points, ..., codes]; 0 where a code has no word"""
    words = prof.words.astype(np.float64)[:, None] * (prof.info_bits > 0)
    return words.reshape((like.shape[0],) + (1,) * (like.ndim - 2) + (-1,))


def _harq_ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def _harq_transmissions(prof):
    """The transmissions used: sum over r of r acked_r, and ``rounds`` for every word never ACKed"""
    r = np.arange(1, 9, dtype=np.float64)
    return (prof.acked.astype(np.float64) * r).sum(axis=-1) + float(prof.rounds) * prof.unacked.astype(np.float64)


def harq_acked(prof):
    """The share of the words ACKed by round r, r = 1 ... rounds: the CDF over the rounds, [points, pairs, n_snr, n_ch, codes,
    rounds]; NaN where a point carried no word"""
    cdf = np.cumsum(prof.acked[..., :prof.rounds].astype(np.float64), axis=-1)
    return _harq_ratio(cdf, _harq_words(prof, prof.unacked)[..., None] * np.ones(prof.rounds))


def harq_mean_transmissions(prof):
    """(sum over r of r acked_r + rounds unacked) / words, shaped as ``unacked``"""
    return _harq_ratio(_harq_transmissions(prof), _harq_words(prof, prof.unacked))


def harq_residual_fer(prof):
    """The share of the words not delivered after the last round: never ACKed, or ACKed with a wrong information bit"""
    return _harq_ratio((prof.unacked + prof.undetected).astype(np.float64), _harq_words(prof, prof.unacked))


def harq_undetected(prof):
    """The share of the words ACKed with a wrong information bit"""
    return _harq_ratio(prof.undetected.astype(np.float64), _harq_words(prof, prof.unacked))


def harq_goodput(prof):
    """Delivered information bits per transmitted coded bit: K (ACKed - undetected) / (n transmissions used)"""
    good = prof.acked.sum(axis=-1).astype(np.float64) - prof.undetected.astype(np.float64)
    lead = (prof.unacked.shape[0],) + (1,) * (prof.unacked.ndim - 2)
    K = prof.info_bits.astype(np.float64).reshape(lead + (-1,))
    n = prof.word_bits.astype(np.float64).reshape(lead + (1,))
    return _harq_ratio(K * good, n * _harq_transmissions(prof))


def harq_bits_per_sample(prof, syms, stride):
    """``harq_goodput`` per on-air sample, so that structures with different symbol lengths compare: a transmission of a frame's W
    words puts W n coded bits on the air in ``syms`` symbols of ``stride`` = B samples each (``Structure.stride``), the known
    symbols and the pilots included"""
    lead = (prof.unacked.shape[0],) + (1,) * (prof.unacked.ndim - 2)
    coded = (prof.frame_words * prof.word_bits).astype(np.float64).reshape(lead + (1,))
    return harq_goodput(prof) * coded / (float(syms) * float(stride))
