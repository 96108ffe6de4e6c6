#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_doppler with 1 and with 4 tracks beside one wofdm_rx_profile call on the same
cells and frames, in the same run -- the shape of tools/bench_rx_profile_sync.py: the half-band system of main_channel_mask.m
at N = 256, 16-QAM, 16 symbols per frame (CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain
and once with the reference's Tx mask.  The channels are channels.gen_channel_tracks' (2 GHz, 5 MHz sampling) at 0, 30, 60
and 100 km/h (f_D = 0, 56, 111, 185 Hz), a knot per symbol stride and S + 2 knots; the plain call runs their knot 0.

Per run: host wall clock around the whole call and the kernels' share of it (HIP events around the chunk loop,
wofdm_rx_profile_kernel_ms) for the plain call, for one track (the 100 km/h one) and for the four; the ratios to the plain
call, and the cost of an additional track in plain calls, (four tracks - one track) / 3.  One JSON line per run, after one
small warm-up call of each.  No threshold: a diagnostic route, not the hot path.

Then, --ser: what the mobility the channel generator names costs, symbol by symbol -- the symbol-error rate per data symbol
s = 1 ... 15 at 0, 50 and 185 Hz for QPSK at 30 dB, and at 50 Hz for 16-QAM at 16 dB (the RC pair, 8 channels), one JSON line
each.

    python tools/bench_rx_profile_doppler.py [--frames 2000] [--ser] [--ser-frames 200]
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
from wofdm_amd import channels as CH  # noqa: E402
from wofdm_amd import rx_profile as R  # noqa: E402

C0, FC, TS = 299792458.0, 2e9, 200e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--ser", action="store_true")
    ap.add_argument("--ser-frames", type=int, default=200)
    args = ap.parse_args()
    n, k, S, pairs, n_ch = 256, 4, 16, 2, 4
    st = W.make_structure("CPW", n, 32)
    B = st.stride
    kmh = [0.0, 30.0, 60.0, 100.0]
    tracks = CH.gen_channel_tracks("vehicularA", n_ch, [v / 3.6 for v in kmh], knot_step=B, n_knots=S + 2,
                                   rng=np.random.RandomState(1)).astype(np.complex64)
    h = np.ascontiguousarray(tracks[0, :, 0])
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    w_tx = np.stack([W.tx_rc_window(st)] * pairs).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st)] * pairs).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    cells = pairs * snr.size * n_ch
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    head = (st, k, S, w_tx, w_rx)
    tail = (snr, 1, 0)
    for name, m in (("plain", None), ("masked", mask)):
        R.rx_profile_gpu(*head, h, *tail, 8, active=alloc, mask=m)                                     # warm-up
        R.rx_profile_doppler_gpu(*head, tracks, B, *tail, 8, active=alloc, mask=m)
        t0 = time.perf_counter()
        alone = R.rx_profile_gpu(*head, h, *tail, args.frames, active=alloc, mask=m)
        wall0 = time.perf_counter() - t0
        ms0 = R.rx_profile_kernel_ms()
        t0 = time.perf_counter()
        one = R.rx_profile_doppler_gpu(*head, tracks[3:], B, *tail, args.frames, active=alloc, mask=m)
        wall1 = time.perf_counter() - t0
        ms1 = R.rx_profile_kernel_ms()
        t0 = time.perf_counter()
        prof = R.rx_profile_doppler_gpu(*head, tracks, B, *tail, args.frames, active=alloc, mask=m)
        wall4 = time.perf_counter() - t0
        ms4 = R.rx_profile_kernel_ms()
        assert np.array_equal(prof.bit_err[0], alone.bit_err)            # the track that holds still is the plain call
        assert np.array_equal(prof.bit_err[3], one.bit_err[0])           # a track does not care what shares its call
        frames = cells * args.frames
        print(json.dumps({
            "what": "wofdm_rx_profile_doppler N=256 16-QAM CPW half-band %s, tracks at %s km/h (2 GHz, 5 MHz), %d knots a stride "
                    "B = %d apart: %d cells x %d frames x %d symbols" % (name, kmh, S + 2, B, cells, args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames_one_track": R.rx_profile_doppler_chunk_frames(st, S, m is not None, 1),
            "chunk_frames_four_tracks": R.rx_profile_doppler_chunk_frames(st, S, m is not None, 4),
            "chunk_frames_plain_call": R.rx_profile_chunk_frames(st, S, m is not None),
            "plain_call_wall_s": wall0, "plain_call_kernels_s": ms0 * 1e-3,
            "one_track_wall_s": wall1, "one_track_kernels_s": ms1 * 1e-3, "one_track_over_plain_kernels": ms1 / ms0,
            "four_tracks_wall_s": wall4, "four_tracks_kernels_s": ms4 * 1e-3, "four_tracks_over_plain_kernels": ms4 / ms0,
            "additional_track_in_plain_calls": (ms4 - ms1) / 3.0 / ms0,
            "frame_tracks_per_s_kernels": frames * 4 / (ms4 * 1e-3),
            "ber_per_track": (prof.bit_err.sum(axis=(1, 2, 3, 4)) / (prof.decisions.sum() * cells * k)).round(5).tolist()}),
            flush=True)
    if not args.ser:
        return
    # the per-symbol cost of the generator's own mobility: RC pair, 8 channels, one SNR point
    hz = [0.0, 50.0, (100 / 3.6) / C0 * FC]
    tr8 = CH.gen_channel_tracks("vehicularA", 8, [f * C0 / FC for f in hz], carrier_frequency=FC, sample_period=TS, knot_step=B,
                                n_knots=S + 2, rng=np.random.RandomState(2)).astype(np.complex64)
    for kk, snr_db, use in ((2, 30.0, (0, 1, 2)), (4, 16.0, (0, 1))):
        prof = R.rx_profile_doppler_gpu(st, kk, S, w_tx[:1], w_rx[:1], tr8[list(use)], B, [snr_db], 3, 0, args.ser_frames,
                                        active=alloc)
        per_symbol = 8 * args.ser_frames * int(np.count_nonzero(alloc))
        print(json.dumps({
            "what": "symbol-error rate per data symbol s = 1 ... %d, CPW N=256 cp=32 half band, RC windows, %d-QAM at %g dB, "
                    "8 Veh-A channels x %d frames" % (S - 1, 1 << kk, snr_db, args.ser_frames),
            "doppler_hz": [round(hz[i], 1) for i in use],
            "ser_per_symbol": (prof.sym_err_sym.sum(axis=(1, 2, 3)) / per_symbol).round(4).tolist()}), flush=True)


if __name__ == "__main__":
    main()
