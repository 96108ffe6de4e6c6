#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_soft beside wofdm_rx_profile_link with the same points, in ONE run -- the
shape of tools/bench_rx_profile_link.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.
Pair 0 is the raised-cosine pair, pair 1 a pair with linear edges (the same tails, straight ramps).

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms), each call made twice and the
second taken:
  - the all-off point and the everything-on point of the link bench (6 dB Rapp, a 185 Hz track, timing +2, cfo 0.02 tracked,
    linewidth 1e-3 tracked, a neighbour at 0 dB), each through wofdm_rx_profile_link and through wofdm_rx_profile_soft with 1, 8 and
    16 scales (the first of the default half-octave list): the ratios to the link call say what the demapper, its scratch and its
    ordered sums cost, and the slope per scale;
  - the chunk lengths of the calls (the soft call's scratch shortens them).
The five link fields of every soft result are compared with the link call's by bytes on the way.  With 16 scales the run also
reports, per pair at the everything-on point, the symbol-error rate and the achievable rate (``gmi``, a scale per bin) averaged
over the cells, and whether the two pairs rank the same way by both.  One JSON line per run.  A diagnostic route, not the hot
path; the boxes switch clock states, so only figures of one run compare.

    python tools/bench_rx_profile_soft.py [--frames 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wofdm_amd as W  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import channels as CH  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    args = ap.parse_args()
    n, k, S, n_ch, fs = 256, 4, 16, 4, 5e6
    st = W.make_structure("CPW", n, 32)
    B = st.stride
    h = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"][:n_ch].astype(np.complex64)
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    lin_tx = W.expand_tx_window(st, np.concatenate(([1.0], np.linspace(1.0, 0.0, st.tail_tx + 2)[1:-1])))
    lin_rx = W.expand_rx_window(st, np.concatenate(([1.0], np.linspace(0.5, 0.0, st.tail_rx // 2 + 2)[1:-1])))
    names = ("rc", "linear")
    w_tx = np.stack([W.tx_rc_window(st), lin_tx]).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st), lin_rx]).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    tracks = np.stack([CH.gen_chan_track("vehicularA", h.shape[1], 185.0, fs, B, S + 2, np.random.RandomState(77 + c))
                       for c in range(n_ch)])[None].astype(np.complex64)
    L, rapp = R.LinkPoint, R.PaPoint(R.PA_RAPP, 6.0, 2.0)
    points = {"all_off": L(), "everything_on": L(rapp, 0, 2, 0.02, 1, 1e-3, 1, (B // 3, 0.0))}
    cells = w_tx.shape[0] * snr.size * n_ch
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    base = (st, k, S, w_tx, w_rx, h, snr, 1, 0)
    for name, m in (("plain", None), ("masked", mask)):
        kw = dict(active=alloc, mask=m)
        ref = R.pa_ref_power(st, k, S, w_tx, 1, 0, 64, active=alloc, mask=m).astype(np.float32)
        side = dict(tracks=tracks, knot_step=B, aci_active=~alloc, ref_power=ref, **kw)

        def timed(call, frames=args.frames):
            call(8)                                                    # warm-up
            call(frames)
            out = call(frames)
            return out, R.rx_profile_kernel_ms()
        res = {}
        for pname, point in points.items():
            link, ms0 = timed(lambda f: R.rx_profile_link_gpu(*base, f, [point], **side))
            res["%s_link_kernels_s" % pname] = ms0 * 1e-3
            ms_of = {}
            for ns in (1, 8, 16):
                soft, ms = timed(lambda f: R.rx_profile_soft_gpu(*base, f, [point], R.SOFT_SCALES[:ns], **side))
                assert all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(soft[:7], link[:7]))
                ms_of[ns] = ms
                res["%s_soft_%d_scales_kernels_s" % (pname, ns)] = ms * 1e-3
                res["%s_soft_%d_scales_over_link" % (pname, ns)] = ms / ms0
            res["%s_per_additional_scale_over_link" % pname] = (ms_of[16] - ms_of[1]) / 15.0 / ms0
            if pname == "everything_on":
                rate = R.gmi(soft, k)[0][0].mean(axis=(1, 2))
                ser = (soft.sym_err[0].sum(axis=-1) / float(soft.decisions.sum())).mean(axis=(1, 2))
                res.update({"everything_on_rate_bit_per_decision": dict(zip(names, np.round(rate, 4).tolist())),
                            "everything_on_symbol_error_rate": dict(zip(names, np.round(ser, 4).tolist())),
                            "pairs_rank_the_same_by_ser_and_by_rate": bool((rate[0] > rate[1]) == (ser[0] < ser[1])),
                            "everything_on_rate_per_snr_rc": np.round(R.gmi(soft, k)[0][0, 0].mean(axis=-1), 3).tolist(),
                            "everything_on_rate_per_snr_linear": np.round(R.gmi(soft, k)[0][0, 1].mean(axis=-1), 3).tolist()})
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_soft N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, one "
                    "point" % (name, st.prefix_rm, st.stride, cells, args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames_link": R.rx_profile_link_chunk_frames(st, S, m is not None, 1, True),
            "chunk_frames_soft_16_scales": R.rx_profile_soft_chunk_frames(st, S, m is not None, 1, True, 16)}, **res)), flush=True)


if __name__ == "__main__":
    main()
