"""Cases, points and mirror references of the power-amplifier receive-profile tests (tests/test_rx_profile_pa_host.py,
tests/test_gpu_rx_profile_pa.py).

The reference is the fp64 host route ``rx_profile_pa_host`` (``frame_profile_pa`` on a linear point is ``frame_profile``,
which tests/test_rx_profile_host.py ties to the CPU oracle).  References are computed once per case and shared (``reference``
is cached); the arrays they return are not to be modified.

A case is one of the seven shapes of tests/doppler_cases.py (``rx_profile_cases.make_case``, its SNR points) behind three
amplifiers in one call: a linear point, a Rapp point with p = 2 and a soft limiter, each at the back-off of ``IBO_DB``.  The
reference power of a pair is the host ``pa_ref_power`` of the case's own frames.  Back-offs and seeds are decided on the CPU
from the mirror alone: it counts errors in every cell, gets fewer than half of a point's decisions wrong
(``check_error_rates``), every amplified point differs from the linear one in every cell, and at most 1 % of a point's
decisions are near ones (``pick_seed``, ``RC.pick_seed``'s cap over 32 seeds -- a condition on the inputs, no tolerance).
"""
import functools

import numpy as np

from wofdm_amd import rx_profile as R

import doppler_cases as DC
import rx_profile_cases as RC

CASES = DC.CASES
#: name -> (back-off of the Rapp point, back-off of the soft limiter) [dB].  Compression adds an error vector of its own on top
#: of the noise's: the cases whose linear point already sits near one half of the decisions (the full-band masked case, whose
#: mask leaves half of the bins to the noise) are backed off further, and so is the 64-QAM case: at (4, 3) dB its mirror got more
#: than half of the decisions of a point wrong.
IBO_DB = {
    "n64_wtx_plain": (3.0, 2.0),
    "n128_wrx_half": (2.0, 1.0),
    "n256_cpw_half_masked": (8.0, 7.0),
    "n512_wola_plain": (3.0, 2.0),
    "n1024_wtx_half_masked": (3.0, 1.5),
    "n128_cpw_half_nbt0": (3.0, 2.0),
    "n64_cp_masked": (8.0, 6.0),
}


def points_of(name):
    rapp, clip = IBO_DB[name]
    return (R.PaPoint(R.PA_LINEAR, 0.0), R.PaPoint(R.PA_RAPP, rapp, 2.0), R.PaPoint(R.PA_CLIP, clip))


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(DC.case(name))                                            # (the shared dict stays as it is)
    c["name"] = name
    c["points"] = points_of(name)
    return c


@functools.lru_cache(maxsize=None)
def ref_power(name, seed, frame_offset=0, frames=RC.FRAMES):
    """[pairs] float32: the mean on-air power per pair over the symbol periods of the frames pair p transmits as cell p"""
    c = case(name)
    return R.pa_ref_power(c["st"], c["k"], c["S"], c["w_tx"], seed, frame_offset, frames, active=c["active"], mask=c["mask"],
                          gpu=False).astype(np.float32)


def host(c, seed, frame_offset, frames, points=None, ref=None):
    """the mirror's profile and its near decisions [points, pairs, n_snr, n_ch]"""
    return R.rx_profile_pa_host(c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, frame_offset, frames,
                                c["points"] if points is None else points,
                                ref_power(c["name"], seed, frame_offset, frames) if ref is None else ref,
                                active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"], with_near=True)


decisions_of = DC.decisions_of


def pick_seed(c, base_seed, frame_offset=0, frames=RC.FRAMES, tries=32, **kw):
    """first seed from base_seed on whose MIRROR profile has at most 1 % near decisions on every point (RC.pick_seed's cap)"""
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
    """the mirror counts errors in every cell on every point, gets fewer than half of a point's decisions wrong, and every
    amplified point differs from the linear one in every cell; returns the symbol-error rates [points, pairs, n_snr, n_ch]"""
    per_cell = decisions_of(c, frames) // (RC.PAIRS * RC.N_SNR * RC.N_CH)
    ser = prof.sym_err.sum(axis=-1) / per_cell
    print("%s: symbol-error rate per point (smallest cell, largest cell, all cells): %s"
          % (tag, [tuple(round(float(v), 4) for v in (s.min(), s.max(), s.mean())) for s in ser]))
    assert (prof.sym_err.sum(axis=-1) > 0).all() and (prof.bit_err.sum(axis=-1) > 0).all(), tag
    assert (ser.mean(axis=(1, 2, 3)) < 0.5).all(), (tag, ser)
    for i in range(1, prof.err_power.shape[0]):
        assert (np.abs(prof.err_power[i] - prof.err_power[0]).max(axis=-1) > 0).all(), (tag, i)
        assert (prof.pa_power[i, ..., 1] < prof.pa_power[i, ..., 0]).all(), (tag, i)
    return ser
