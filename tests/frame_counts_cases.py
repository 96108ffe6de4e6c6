"""Small launches of the frame kernels whose four counters are pinned to recorded values (tests/test_gpu_counts_pinned.py;
recorded by tests/golden/make_frame_counts_parent.py into tests/golden/frame_counts_parent.npz).

Every case is 2 SNR cells (-5 and 20 dB) x 8 frames of S = 16 symbols, from frame offset 0 and from an offset above 2^32: S = 16 and
more than one cell are the smallest shapes that take the pilot wave, the trailing tile and the per-cell refill of the tables."""
import numpy as np

import kernel_cases as KC
import wofdm_amd as W
from test_geo_table import header_names
from wofdm_amd import channel_mask as CM

SEED = 0x9E3779B97F4A7C15
S, TAPS, FRAMES = 16, 21, 8
SNRS = np.array([-5.0, 20.0], np.float32)
OFFSETS = (0, 2 ** 32 + 5)
STRUCTURES = header_names()                       # the seven rows of wofdm_geo_table (N = 256, CP 32, S = 16)

#: name -> (system, n_fft, cp, k, what): what = "built" | "generic" | "plain" | "allocation" | "mask"
CASES = {}
for _s in STRUCTURES:
    CASES["built-%s-k4" % _s] = (_s, 256, 32, 4, "built")
    CASES["generic-%s-k4" % _s] = (_s, 256, 32, 4, "generic")
for _k in (2, 6):
    CASES["built-wtx-k%d" % _k] = ("wtx", 256, 32, _k, "built")
for _n, _lay in ((64, 13), (128, 13), (512, 12), (1024, 12)):
    _sys, _cp, _S, _opt = KC.geometry_for(_n, _lay, 0)
    assert _S == S and not _opt
    CASES["plain-N%d" % _n] = (_sys, _n, _cp, 4, "plain")
CASES["allocation-N256"] = ("wtx", 256, 32, 4, "allocation")
CASES["mask-N256"] = ("wtx", 256, 32, 4, "mask")


def run_case(name, channels):
    """[len(OFFSETS)] arrays of counters [channel][snr][window][4] of case `name` on cuda:0."""
    system, n_fft, cp, k, what = CASES[name]
    st = W.make_structure(system, n_fft, cp)
    cfg = W.make_cfg(st, k, S, TAPS, 1, len(SNRS), 1, seed=SEED)
    with W.Plan(cfg, W.tx_rc_window(st).astype(np.float32), W.rx_rc_window(st).astype(np.float32),
                channels[11:12].astype(np.complex64), SNRS) as plan:
        if what == "generic":
            plan.set_option("generic_geometry", 1)
        if what == "allocation":
            active = np.ones(n_fft, bool)
            active[1::3] = False
            plan.set_allocation(active)
        if what == "mask":
            plan.set_tx_mask(CM.tx_mask(st.sym_len, roll_off=10))
        if what == "built":
            assert plan.kernel_geo() > 0
        else:
            assert plan.kernel_geo() == 0
        return [plan.run(off, FRAMES).copy() for off in OFFSETS]
