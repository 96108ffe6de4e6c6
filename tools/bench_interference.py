"""Wall time of the closed-form interference entry points, incl. allocation and copies (run from the repository root):
``wofdm_interference`` on 7 window pairs x 100 channels, and the masked leg -- ``wofdm_interference_masked`` with half-band
loading + the raised-cosine Tx mask on the same jobs, and on 7 pairs x 1 channel (the masked pulses are formed once per
pair, so 100 channels must cost far less than 100 x one).  A warm-up call, then REPEATS timed calls; the median counts.

    python tools/bench_interference.py [N ...]      (default: 256 1024)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import wofdm_amd as W  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import interference as I  # noqa: E402

REPEATS = 7
ch = np.load("tests/golden/channels_vehA.npz")["h"]


def median_ms(fn):
    fn()                                             # warm-up: code object load, first allocation
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


for n_fft in [int(a) for a in sys.argv[1:]] or [256, 1024]:
    st = W.make_structure("WOLA", n_fft, 32)
    w_tx = np.tile(W.tx_rc_window(st), (7, 1))
    w_rx = np.tile(W.rx_rc_window(st), (7, 1))
    alloc, mask = CM.half_band_allocation(n_fft), CM.tx_mask(st.sym_len)
    plain = median_ms(lambda: I.interf_power_gpu(st, w_tx, w_rx, ch[:100]))
    if n_fft == 256:
        print("f2 on the GPU: 7 window pairs x 100 channels at N=256 (700 evaluations) in %.1f ms incl. alloc/copies -> the "
              "reference's 26 400 evaluations: %.2f s" % (plain[0], plain[0] * 1e-3 * 26400 / 700))
    m100 = median_ms(lambda: I.interf_power_masked_gpu(st, w_tx, w_rx, ch[:100], active=alloc, mask=mask))
    m1 = median_ms(lambda: I.interf_power_masked_gpu(st, w_tx, w_rx, ch[:1], active=alloc, mask=mask))
    a100 = median_ms(lambda: I.interf_power_masked_gpu(st, w_tx, w_rx, ch[:100], active=alloc))
    print("N=%d WOLA cp 32, 7 pairs, median of %d (min .. max) ms:" % (n_fft, REPEATS))
    print("  wofdm_interference, 100 channels (fully loaded, no mask)   %8.2f (%.2f .. %.2f)" % plain)
    print("  wofdm_interference_masked, 100 channels, half-band + mask  %8.2f (%.2f .. %.2f)   %.2f x the plain call"
          % (m100 + (m100[0] / plain[0],)))
    print("  wofdm_interference_masked, 100 channels, half-band only    %8.2f (%.2f .. %.2f)" % a100)
    print("  wofdm_interference_masked, 1 channel, half-band + mask     %8.2f (%.2f .. %.2f)   100 channels cost %.1f x this"
          % (m1 + (m100[0] / m1[0],)))
