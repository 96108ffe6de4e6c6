"""Cases and references of the geometry-limit tests (tests/test_edge_geometry_host.py, tests/test_gpu_edge_geometry.py).

include/wofdm.h documents for ``wofdm_rx_profile`` and its descendants n_taps 1 ... 21, tail_rx even and up to 64, cp and cs up to
n_fft, 2 tail_tx <= P and any prefix_rm / circ_shift with n_fft + tail_rx + prefix_rm == P - tail_tx; ``wofdm_plan_create`` takes
tail_rx <= 64, tail_tx <= 16 and a stride of at most n_fft + 64.  The other case modules stay at the reference's tails (8 / 10), 21
taps, cp = N / 8 and a circ_shift of at most 5; the eleven geometries of ``CASES`` sit on the documented limits instead.

A case is ``rx_profile_cases.make_case``'s (2 pairs x 2 SNR points x 2 channels x 8 frames, random windows of the case's own tails)
with the channels cut to the case's taps and 0.5 added to tap 0, as tests/test_gpu_fuzz.py keeps short channels away from deep
nulls.  The reference is the CPU oracle (``rx_profile_cases.oracle_profile``); the seed of a case is the first of 32 from
``BASE_SEED`` for which the oracle alone has at most 1 % near decisions (``rx_profile_cases.pick_seed``).  k and the two SNR points
of a case are chosen on the CPU from the oracle alone: it counts bit and symbol errors in every pair at both points and gets fewer
than half of the decisions wrong at the upper one (``check_error_rates``).

Three cases (``LINK_CASES``) also carry two points of the combined chain, everything on: a 6 dB Rapp amplifier, track 1 -- 185 Hz,
knot_step 37 (it divides nothing), knots over the frame and one stride more --, carrier offset and linewidth tracked at one point
and free-running at the other, a neighbour on the complementary allocation.  Point 0 has timing -(prefix_rm + 3), so its first
window begins before the frame, and a neighbour delay of B - 1; point 1 timing +5 and delay 0.  Their reference is the fp64 mirror
``rx_profile_link_host``, their seed the first of 32 for which the MIRROR has at most 1 % near decisions at both points
(tests/test_gpu_rx_profile_link.py's rule).  ``fold_all_n64`` also runs the tracking receiver (1, 1) on the same two points behind
a comb of every eighth loaded bin, against ``rx_profile_tracking_host`` under tests/test_gpu_rx_profile_tracking.py's seed rule.

References are computed once per case and shared (cached); the arrays they return are not to be modified.
"""
import functools

import numpy as np

import wofdm_amd as W
from wofdm_amd import channel_mask as CM
from wofdm_amd import rx_profile as R

import doppler_cases as DC
import kernel_cases as KC
import rx_profile_cases as RC

L, TP = R.LinkPoint, R.TrackingPoint
RAPP6 = R.PaPoint(R.PA_RAPP, 6.0, 2.0)
BASE_SEED = 100
KNOT_STEP = 37

#: name -> (system, n_fft, cp, tail_tx, tail_rx, S, taps, variant, k, the two SNR points [dB], noise_before_truncate, the frame
#: kernels take it).  What each reaches:
#:   fold_all_n64     P = 192, B - N = 96, tail_rx = N: every sample of the window folds, the receive kernel's row is filled to N + 84
#:                    of its N + 88 samples, cp = cs = n_fft
#:   plan_n1024_wrx   B - N = 64 with prefix_rm = 0, cp + cs = 64: the frame kernels' limit at N = 1024
#:   plan_n128_wola   tail_tx = 16 and tail_rx = 64 together, circ_shift = 32, 5 taps, S no multiple of the wave
#:   plan_n256_cpw    stride 320: 4 B = 1280, the last stride layout 11 takes
#:   cpwtx_n256       CPwtx, circ_shift = 48, cs = prefix_rm = 0, B = N, a Tx tail six times the reference's, masked
#:   plan_n512_cpwrx  CPwrx, circ_shift = 32, one tap, S = 2
#:   txtail_n64       tail_tx = 64 of P = 144 (the 2 tail_tx <= P side), cs = n_fft, two taps
#:   cpfull_n128      cp = n_fft, prefix_rm = 128, 20 taps, masked
#:   tiny_n256        a prefix far shorter than the channel: the 20 samples of history come from the previous symbol
#:   rm0_n64          cp = cs = 1, prefix_rm = 0, B = 66
#:   odd_n512_cpw     odd cp, odd tail_tx, tail_rx / 2 odd, masked
#: k and the SNR points are RC.SNR_DB's 16-QAM at 8 / 16 dB or QPSK at 0 / 8 dB where the oracle meets ``check_error_rates`` with
#: them.  64-QAM sits on the two cases without intersymbol interference (one tap; cp = n_fft), at points of its own: on
#: plan_n128_wola it has an error floor of one half whatever the SNR, and on plan_n256_cpw a symbol-error rate of 0.6 ... 0.8.
#: fold_all_n64 runs QPSK at 4 / 12 dB: with 16-QAM its link point whose window begins before the frame gets three quarters of
#: the decisions wrong with carrier offset, linewidth and neighbour all off.  The figures: profiles/edge_geometry.txt, 0.
CASES = {
    "fold_all_n64": ("CPW", 64, 64, 32, 64, 5, 21, "plain", 2, (4.0, 12.0), 1, False),
    "plan_n1024_wrx": ("wrx", 1024, 32, 0, 64, 5, 21, "half", 4, (8.0, 16.0), 1, True),
    "plan_n128_wola": ("WOLA", 128, 64, 16, 64, 9, 5, "half", 4, (8.0, 16.0), 1, True),
    "plan_n256_cpw": ("CPW", 256, 32, 8, 64, 16, 21, "plain", 2, (0.0, 8.0), 0, True),
    "cpwtx_n256": ("CPwtx", 256, 48, 48, 0, 4, 21, "half_masked", 2, (0.0, 8.0), 1, False),
    "plan_n512_cpwrx": ("CPwrx", 512, 64, 0, 64, 2, 1, "plain", 6, (12.0, 20.0), 1, True),
    "txtail_n64": ("wtx", 64, 16, 64, 0, 16, 2, "half", 2, (0.0, 8.0), 1, False),
    "cpfull_n128": ("CP", 128, 128, 0, 0, 7, 20, "half_masked", 6, (14.0, 22.0), 0, False),
    "tiny_n256": ("wtx", 256, 2, 2, 0, 13, 21, "plain", 2, (0.0, 8.0), 1, True),
    "rm0_n64": ("wrx", 64, 1, 0, 2, 3, 3, "plain", 4, (8.0, 16.0), 0, True),
    "odd_n512_cpw": ("CPW", 512, 33, 7, 18, 3, 21, "half_masked", 4, (8.0, 16.0), 1, True),
}
PLAN_CASES = tuple(n for n, v in CASES.items() if v[-1])
REFUSED_CASES = tuple(n for n, v in CASES.items() if not v[-1])
#: name -> (cfo, linewidth, the neighbour's level at point 0 and at point 1 [dB]).  tests/test_gpu_rx_profile_link.py's levels are
#: 0.02, 1e-3, 0 / -6 dB; they are lowered where the MIRROR got half or more of a point's decisions wrong at the upper SNR point
#: with them: 0.76 at the free-running point of plan_n128_wola (16-QAM), 0.52 at that of fold_all_n64.
LINK_CASES = {
    "fold_all_n64": (0.01, 1e-3, -6.0, -12.0),
    "plan_n128_wola": (0.005, 1e-3, 0.0, -6.0),
    "cpwtx_n256": (0.02, 1e-3, 0.0, -6.0),
}
TRACKING_CASE = "fold_all_n64"
TRACKING_SCALES = (0.5,)


def structure(name):
    system, n, cp, btx, brx = CASES[name][:5]
    return W.make_structure(system, n, cp, btx, brx)


def plan_var(c):
    """``kernel_cases.expected_kernel_id``'s var of a case: nothing set, an allocation, a Tx mask"""
    return KC.VAR_TXMASK if c["mask"] is not None else KC.VAR_ALLOC if c["active"] is not None else KC.VAR_PLAIN


@functools.lru_cache(maxsize=None)
def case(name):
    S, taps, variant, k, snr, nbt = CASES[name][5:11]
    c = RC.make_case(structure(name), k, S, variant, 9000 + list(CASES).index(name), nbt)
    h = c["h"][:, :taps].copy()
    h[:, 0] += 0.5                                        # keep short channels away from deep nulls
    c.update(name=name, h=h, snr=np.array(snr, np.float32))
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, seed, oracle profile of the frames [0, RC.FRAMES))"""
    c = case(name)
    seed, ref = RC.pick_seed(c, BASE_SEED)
    return c, seed, ref


def check_error_rates(c, bit, sym, decisions, tag=""):
    """bit, sym [..., pairs, n_snr, n_ch, N]: errors are counted in every pair at both SNR points, and fewer than half of the
    decisions are wrong at the upper point (on every leading index); returns the symbol-error rates [..., n_snr]"""
    b, s = bit.sum(axis=(-1, -2)), sym.sum(axis=(-1, -2))                # [..., pairs, n_snr]
    ser = s.sum(axis=-2) / (decisions / RC.N_SNR)
    print("%s: symbol-error rate at the two SNR points %s" % (tag, np.round(ser, 4)))
    assert (b > 0).all() and (s > 0).all(), (tag, b, s)
    assert (ser[..., 1] < 0.5).all(), (tag, ser)
    return ser


# ---- the combined chain ----

@functools.lru_cache(maxsize=None)
def link_case(name):
    c = dict(case(name))                                                # (the shared dict stays as it is)
    st, S = c["st"], c["S"]
    B = st.stride
    cfo, lw, lvl0, lvl1 = LINK_CASES[name]
    n_knots = -(-(st.frame_len(S) + B) // KNOT_STEP) + 1
    assert (n_knots - 1) * KNOT_STEP >= st.frame_len(S) + c["h"].shape[1] - 2 + 5 and n_knots <= 64 and B % KNOT_STEP != 0
    c["knot_step"] = KNOT_STEP
    c["tracks"] = DC.tracks_of(c, (0.0, 185.0 * B / DC.FS), KNOT_STEP, n_knots)
    c["aci_active"] = CM.half_band_allocation(st.n_fft) if c["active"] is None else ~np.asarray(c["active"], bool)
    c["points"] = [L(RAPP6, 1, -(st.prefix_rm + 3), cfo, 1, lw, 1, (B - 1, lvl0)), L(RAPP6, 1, 5, cfo, 0, lw, 0, (0, lvl1))]
    return c


@functools.lru_cache(maxsize=None)
def ref_power(name, seed):
    c = case(name)
    return R.pa_ref_power(c["st"], c["k"], c["S"], c["w_tx"], seed, 0, RC.FRAMES, active=c["active"], mask=c["mask"],
                          gpu=False).astype(np.float32)


def link_sides(c, seed):
    return dict(tracks=c["tracks"], knot_step=c["knot_step"], aci_active=c["aci_active"], ref_power=ref_power(c["name"], seed),
                active=c["active"], mask=c["mask"], noise_before_truncate=c["nbt"])


def head(c, seed):
    return (c["st"], c["k"], c["S"], c["w_tx"], c["w_rx"], c["h"], c["snr"], seed, 0, RC.FRAMES)


@functools.lru_cache(maxsize=None)
def link_reference(name, tries=32):
    """(case, seed, the mirror's profile, its near decisions [points, pairs, n_snr, n_ch])"""
    c = link_case(name)
    for seed in range(BASE_SEED, BASE_SEED + tries):
        prof, near = R.rx_profile_link_host(*head(c, seed), c["points"], with_near=True, **link_sides(c, seed))
        if (near.sum(axis=(1, 2, 3)) <= 0.01 * DC.decisions_of(c, RC.FRAMES)).all():
            return c, seed, prof, near
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (BASE_SEED, BASE_SEED + tries))


@functools.lru_cache(maxsize=None)
def tracking_case():
    c = dict(link_case(TRACKING_CASE))
    on = np.ones(c["st"].n_fft, bool) if c["active"] is None else np.asarray(c["active"]) != 0
    c["on"], c["pilots"] = on, R.pilot_comb(on, 8)
    c["tracking"] = [TP(1, 1)] * len(c["points"])
    return c


@functools.lru_cache(maxsize=None)
def tracking_reference(tries=32):
    """(case, seed, the mirror's profile, its near decisions [points, pairs, n_snr, n_ch])"""
    c = tracking_case()
    cells = RC.PAIRS * RC.N_SNR * RC.N_CH
    for seed in range(BASE_SEED, BASE_SEED + tries):
        prof, near = R.rx_profile_tracking_host(*head(c, seed), c["points"], c["tracking"], c["pilots"], TRACKING_SCALES,
                                                with_near=True, **link_sides(c, seed))
        if (near.sum(axis=(1, 2, 3)) <= 0.01 * cells * prof.decisions.sum(axis=-1).astype(np.float64)).all():
            return c, seed, prof, near
    raise AssertionError("no seed in [%d, %d) keeps the mirror's decisions clear of the thresholds" % (BASE_SEED, BASE_SEED + tries))
