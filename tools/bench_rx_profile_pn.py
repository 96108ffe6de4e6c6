#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_pn beside one wofdm_rx_profile call on the same cells and frames -- the
shape of tools/bench_rx_profile_sync.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.

Per run: host wall clock around the whole call and the kernels' share of it (HIP events around the chunk loop,
wofdm_rx_profile_kernel_ms) for one point (linewidth 1e-2, free-running), for four points and for the plain call, and the
kernel time per additional point over the plain call's -- the Tx chain, the power pass and the phase walk of a frame run once
for all its points.  And what the phase noise does to the receiver that equalises with the pilot of symbol 0: the symbol-error
rate on the first and on the fifteenth data symbol at linewidths 0, 1e-3 and 1e-2 of a subcarrier spacing, free-running and with
the common phase error tracked (six points, one call; all cells, i.e. all eight SNR points, together).  One JSON line per run,
after one small warm-up call of each.  A diagnostic route, not the hot path.

    python tools/bench_rx_profile_pn.py [--frames 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wofdm_amd as W  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    args = ap.parse_args()
    n, k, S, pairs, n_ch = 256, 4, 16, 2, 4
    st = W.make_structure("CPW", n, 32)
    h = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                             "channels_vehA.npz"))["h"][:n_ch].astype(np.complex64)
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    w_tx = np.stack([W.tx_rc_window(st)] * pairs).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st)] * pairs).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    one = [R.PnPoint(1e-2, 0)]
    four = [R.PnPoint(1e-2, 0), R.PnPoint(1e-2, 1), R.PnPoint(1e-3, 0), R.PnPoint(0.0, 0)]
    rates = [R.PnPoint(b, t) for b in (0.0, 1e-3, 1e-2) for t in (0, 1)]
    cells = pairs * snr.size * n_ch
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    base = (st, k, S, w_tx, w_rx, h, snr, 1, 0)
    for name, m in (("plain", None), ("masked", mask)):
        R.rx_profile_gpu(*base, 8, active=alloc, mask=m)                                               # warm-up
        R.rx_profile_pn_gpu(*base, 8, four, active=alloc, mask=m)
        t0 = time.perf_counter()
        alone = R.rx_profile_gpu(*base, args.frames, active=alloc, mask=m)
        wall0 = time.perf_counter() - t0
        ms0 = R.rx_profile_kernel_ms()
        R.rx_profile_pn_gpu(*base, args.frames, one, active=alloc, mask=m)
        ms1 = R.rx_profile_kernel_ms()
        t0 = time.perf_counter()
        prof = R.rx_profile_pn_gpu(*base, args.frames, four, active=alloc, mask=m)
        wall = time.perf_counter() - t0
        ms4 = R.rx_profile_kernel_ms()
        assert np.array_equal(prof.bit_err[3], alone.bit_err)            # the point of linewidth 0 is the plain call
        assert prof.err_power[3].tobytes() == alone.err_power.tobytes()
        swp = R.rx_profile_pn_gpu(*base, args.frames, rates, active=alloc, mask=m)
        # symbol errors of data symbol s over the loaded bins of all cells and frames
        per_sym = swp.sym_err_sym.sum(axis=(1, 2, 3)) / float(cells * args.frames * np.count_nonzero(alloc))
        frames = cells * args.frames
        print(json.dumps({
            "what": "wofdm_rx_profile_pn N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames_4_points": R.rx_profile_pn_chunk_frames(st, S, m is not None, 4),
            "chunk_frames_plain_call": R.rx_profile_chunk_frames(st, S, m is not None),
            "plain_call_wall_s": wall0, "plain_call_kernels_s": ms0 * 1e-3,
            "one_point_kernels_s": ms1 * 1e-3, "one_point_over_plain_kernels": ms1 / ms0,
            "four_points_wall_s": wall, "four_points_kernels_s": ms4 * 1e-3, "four_points_over_plain_kernels": ms4 / ms0,
            "per_additional_point_over_plain_kernels": (ms4 - ms1) / 3.0 / ms0,
            "frame_points_per_s_kernels_4_points": frames * 4 / (ms4 * 1e-3),
            "ser_points_linewidth_tracked": [tuple(q) for q in rates],
            "ser_first_data_symbol": per_sym[:, 0].round(5).tolist(),
            "ser_fifteenth_data_symbol": per_sym[:, S - 2].round(5).tolist()}), flush=True)


if __name__ == "__main__":
    main()
