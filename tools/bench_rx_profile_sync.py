#!/usr/bin/env python3
"""Developer tool (GPU box): time a wofdm_rx_profile_sync sweep beside one wofdm_rx_profile call on the same cells and frames
-- the shape of tools/bench_rx_profile.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per
frame (CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx
mask; the sweep is BER against timing offset: 9 timing points from before the prefix to past the suffix, no carrier offset.

Per run: host wall clock around the whole call and the kernels' share of it (HIP events around the chunk loop,
wofdm_rx_profile_kernel_ms) for the sweep and for the plain call, and the sweep's kernel time per point over the plain call's
-- below 1 is the expectation: the Tx chain and the power pass of a frame run once for all its points.  A one-point sweep is
timed as well: what the rotation and the per-symbol sums cost a single point.  One JSON line per run, after one small warm-up
call of each.  A diagnostic route, not the hot path.

    python tools/bench_rx_profile_sync.py [--frames 2000]
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
    timings = [int(t) for t in np.linspace(-(st.prefix_rm + 8), st.cs + 8, 9).round()]
    points = [R.SyncPoint(t) for t in timings]
    assert 0 in timings and len(points) == 9
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
        R.rx_profile_sync_gpu(*base, 8, points, active=alloc, mask=m)
        t0 = time.perf_counter()
        alone = R.rx_profile_gpu(*base, args.frames, active=alloc, mask=m)
        wall0 = time.perf_counter() - t0
        ms0 = R.rx_profile_kernel_ms()
        t0 = time.perf_counter()
        prof = R.rx_profile_sync_gpu(*base, args.frames, points, active=alloc, mask=m)
        wall = time.perf_counter() - t0
        ms = R.rx_profile_kernel_ms()
        R.rx_profile_sync_gpu(*base, args.frames, [R.SyncPoint(0)], active=alloc, mask=m)
        ms1 = R.rx_profile_kernel_ms()
        i0 = timings.index(0)
        assert np.array_equal(prof.bit_err[i0], alone.bit_err)           # the point without offsets is the plain call
        frames = cells * args.frames
        print(json.dumps({
            "what": "wofdm_rx_profile_sync N=256 16-QAM CPW half-band %s, %d timing points %s (gamma = %d, cs = %d, B = %d): "
                    "%d cells x %d frames x %d symbols" % (name, len(points), timings, st.prefix_rm, st.cs, st.stride, cells,
                                                           args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": R.rx_profile_sync_chunk_frames(st, S, m is not None, len(points)),
            "chunk_frames_plain_call": R.rx_profile_chunk_frames(st, S, m is not None),
            "wall_s": wall, "kernels_s": ms * 1e-3, "frame_points_per_s_kernels": frames * len(points) / (ms * 1e-3),
            "plain_call_wall_s": wall0, "plain_call_kernels_s": ms0 * 1e-3,
            "sweep_over_plain_kernels": ms / ms0, "sweep_per_point_over_plain_kernels": ms / ms0 / len(points),
            "one_point_sweep_kernels_s": ms1 * 1e-3, "one_point_sweep_over_plain_kernels": ms1 / ms0,
            "ber_per_timing_point": (prof.bit_err.sum(axis=(1, 2, 3, 4)) / (prof.decisions.sum() * cells * k)).round(5).tolist()}),
            flush=True)


if __name__ == "__main__":
    main()
