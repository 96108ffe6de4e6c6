"""Cases, tracks and mirror references of the moving-channel receive-profile tests (tests/test_rx_profile_doppler_host.py,
tests/test_gpu_rx_profile_doppler.py).

The reference is the fp64 host route ``rx_profile_doppler_host`` (``frame_profile_doppler`` on a static track is
``frame_profile``, which tests/test_rx_profile_host.py ties to the CPU oracle).  References are computed once per case and
shared (``reference`` is cached); the arrays they return are not to be modified.

A case runs three tracks with knot_step = B and S + 2 knots: the static track of the case's channels, and the same channel
index moving at two Doppler values nu, in cycles per symbol period (f_D = nu fs / B), from ``channels.gen_chan_track`` -- one
realisation per channel, the same oscillator phases at both values.  nu is chosen per case so that the mirror counts errors in
every cell and gets fewer than half of a track's decisions wrong (``check_error_rates``; the share of the track that holds
still is the SNR's, ``PARAMS``).  The reference's own 185 Hz at N = 256, 5 MHz is nu = 0.011.
"""
import functools

import numpy as np

import wofdm_amd as W
from wofdm_amd import channels as CH
from wofdm_amd import rx_profile as R

import rx_profile_cases as RC

FS = 5e6
#: name -> (n_fft, system, cp, k, S, variant, nbt): the shapes of tests/test_gpu_rx_profile_sync.py
CASES = {
    "n64_wtx_plain": (64, "wtx", 8, 2, 4, "plain", 1),
    "n128_wrx_half": (128, "wrx", 16, 2, 9, "half", 1),
    "n256_cpw_half_masked": (256, "CPW", 32, 6, 16, "half_masked", 1),
    "n512_wola_plain": (512, "WOLA", 64, 4, 3, "plain", 1),
    "n1024_wtx_half_masked": (1024, "wtx", 128, 4, 2, "half_masked", 1),
    "n128_cpw_half_nbt0": (128, "CPW", 32, 4, 4, "half", 0),
    "n64_cp_masked": (64, "CP", 16, 4, 5, "masked", 1),
}
#: name -> (the two SNR points [dB], the two Doppler values [cycles per symbol period]).  The SNR points are higher than
#: RC.SNR_DB's where a channel that holds still already gets half of a cell's decisions wrong there; on the full band the Tx
#: mask leaves half of the bins to the noise whatever the SNR, so n64_cp_masked stays near one half on the track that holds still.
PARAMS = {
    "n64_wtx_plain": ((4.0, 10.0), (0.01, 0.03)),
    "n128_wrx_half": ((0.0, 8.0), (0.004, 0.012)),
    "n256_cpw_half_masked": ((16.0, 22.0), (0.001, 0.002)),
    "n512_wola_plain": ((12.0, 18.0), (0.008, 0.02)),
    "n1024_wtx_half_masked": ((10.0, 18.0), (0.02, 0.04)),
    "n128_cpw_half_nbt0": ((8.0, 16.0), (0.005, 0.015)),
    "n64_cp_masked": ((14.0, 22.0), (0.002, 0.004)),
}
NU = {name: v[1] for name, v in PARAMS.items()}
#: the case that also runs a step that divides nothing, a two-knot track over the whole frame and a 64-knot track
EXTRA = "n64_wtx_plain"


def tracks_of(c, nus, knot_step, n_knots, seed=77):
    """[len(nus), n_ch, n_knots, taps] complex64: per channel index one GMEDS_1 realisation (rng seed + channel) at the Doppler
    values ``nus`` (cycles per symbol period B); nu = 0 is the case's own channel, held"""
    st, h = c["st"], c["h"]
    out = np.zeros((len(nus), h.shape[0], n_knots, h.shape[1]), np.complex64)
    for i, nu in enumerate(nus):
        for ch in range(h.shape[0]):
            out[i, ch] = (np.tile(h[ch], (n_knots, 1)) if nu == 0.0 else
                          CH.gen_chan_track("vehicularA", h.shape[1], nu * FS / st.stride, FS, knot_step, n_knots,
                                            np.random.RandomState(seed + ch)))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    n, system, cp, k, S, variant, nbt = CASES[name]
    c = RC.make_case(W.make_structure(system, n, cp), k, S, variant, 6000 + n + len(name), nbt)
    c["snr"] = np.array(PARAMS[name][0], np.float32)
    c["knot_step"] = c["st"].stride
    c["tracks"] = tracks_of(c, (0.0,) + NU[name], c["st"].stride, S + 2)
    return c


def extra_tracks(c):
    """[(tracks [1 or 2, n_ch, n_knots, taps], knot_step)]: a step that divides nothing (37, as many knots as cover the frame); two
    knots whose single interval ends on the last sample of conv (there a div knot_step = 1 meets the clamp on q: noise_before_truncate
    = 1, so pass 1 takes that sample); 64 knots"""
    st, S, nu = c["st"], c["S"], NU[EXTRA][1]
    last = st.frame_len(S) + c["h"].shape[1] - 2
    k37 = -(-last // 37) + 1
    assert 2 <= k37 <= 64
    k64 = -(-last // 63)
    assert c["nbt"] == 1
    out = [(tracks_of(c, (0.0, nu), 37, k37), 37), (tracks_of(c, (nu,), last, 2), last), (tracks_of(c, (0.0, nu), k64, 64), k64)]
    return out


def host(c, seed, frame_offset, frames, tracks=None, knot_step=None):
    """the mirror's profile and its near decisions [tracks, pairs, n_snr, n_ch]"""
    return R.rx_profile_doppler_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["tracks"] if tracks is None else tracks,
                                     c["knot_step"] if knot_step is None else knot_step, c["snr"], seed, frame_offset, frames,
                                     active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], with_near=True)


def decisions_of(c, frames):
    n_on = c["st"].n_fft if c["active"] is None else int(np.count_nonzero(c["active"]))
    return RC.PAIRS * RC.N_SNR * RC.N_CH * frames * (c["S"] - 1) * n_on


def pick_seed(c, base_seed, frame_offset=0, frames=RC.FRAMES, tries=32, **kw):
    """first seed from base_seed on whose MIRROR profile has at most 1 % near decisions on every track (RC.pick_seed's cap)"""
    for seed in range(base_seed, base_seed + tries):
        prof, near = host(c, seed, frame_offset, frames, **kw)
        if (near.sum(axis=(1, 2, 3)) <= 0.01 * decisions_of(c, frames)).all():
            return seed, prof, near
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (base_seed, base_seed + tries))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    seed, prof, near = pick_seed(c, 100 * (1 + list(CASES).index(name)))
    return c, seed, prof, near


def check_error_rates(c, prof, frames, tag=""):
    """the mirror counts errors in every cell on every track, and gets fewer than half of a track's decisions wrong; returns
    the symbol-error rates [tracks, pairs, n_snr, n_ch]"""
    per_cell = decisions_of(c, frames) // (RC.PAIRS * RC.N_SNR * RC.N_CH)
    ser = prof.sym_err.sum(axis=-1) / per_cell
    print("%s: symbol-error rate per track (smallest cell, largest cell, all cells): %s"
          % (tag, [tuple(round(float(v), 4) for v in (s.min(), s.max(), s.mean())) for s in ser]))
    assert (prof.sym_err.sum(axis=-1) > 0).all() and (prof.bit_err.sum(axis=-1) > 0).all(), tag
    assert (ser.mean(axis=(1, 2, 3)) < 0.5).all(), (tag, ser)
    return ser
