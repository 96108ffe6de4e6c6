#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_pa with 1 and with 4 points beside one wofdm_rx_profile call on the same
cells and frames, in the same run -- the shape of tools/bench_rx_profile_doppler.py: the half-band system of main_channel_mask.m
at N = 256, 16-QAM, 16 symbols per frame (CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain
and once with the reference's Tx mask.  The points: a linear one, the Rapp model (p = 2) at 6 and at 3 dB of back-off, the
soft limiter at 3 dB; the one-point call runs Rapp at 3 dB.  The back-off counts from rx_profile.pa_ref_power of 200 frames.

Per run: host wall clock around the whole call and the kernels' share of it (HIP events around the chunk loop,
wofdm_rx_profile_kernel_ms) for the plain call, for one point and for the four; the ratios to the plain call, and the cost of
an additional point in plain calls, (four points - one point) / 3.  One JSON line per run, after one small warm-up call of
each.  No threshold: a diagnostic route, not the hot path.

Then, --physical: what the back-off costs and what it gives back -- for the RC pair, plain and masked, at 9, 6 and 3 dB
behind the Rapp amplifier (p = 2) and without one: the symbol-error rate at 30 dB over the 4 channels
(wofdm_rx_profile_pa) and the out-of-band radiation of 256 symbols of 16-QAM on the half band, over the in-band mean
(wofdm_tx_psd_batch_pa); one JSON line.

    python tools/bench_rx_profile_pa.py [--frames 2000] [--physical] [--physical-frames 200] [--out FILE]

profiles/rx_profile_pa.txt holds the lines of one run (--out appends them to a file as well as printing them).
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
from wofdm_amd import rx_profile as R  # noqa: E402
from wofdm_amd import timefreq as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--physical", action="store_true")
    ap.add_argument("--physical-frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    n, k, S, pairs, n_ch = 256, 4, 16, 2, 4
    st = W.make_structure("CPW", n, 32)
    h = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"][:n_ch].astype(np.complex64)
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    w_tx = np.stack([W.tx_rc_window(st)] * pairs).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st)] * pairs).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    cells = pairs * snr.size * n_ch
    pts = [R.PaPoint(R.PA_LINEAR, 0.0), R.PaPoint(R.PA_RAPP, 6.0, 2.0), R.PaPoint(R.PA_RAPP, 3.0, 2.0), R.PaPoint(R.PA_CLIP, 3.0)]
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    head = (st, k, S, w_tx, w_rx, h, snr, 1, 0)
    for name, m in (("plain", None), ("masked", mask)):
        ref = R.pa_ref_power(st, k, S, w_tx, 1, 0, 200, active=alloc, mask=m)
        R.rx_profile_gpu(*head, 8, active=alloc, mask=m)                                               # warm-up
        R.rx_profile_pa_gpu(*head, 8, pts, ref, active=alloc, mask=m)
        t0 = time.perf_counter()
        alone = R.rx_profile_gpu(*head, args.frames, active=alloc, mask=m)
        wall0 = time.perf_counter() - t0
        ms0 = R.rx_profile_kernel_ms()
        t0 = time.perf_counter()
        one = R.rx_profile_pa_gpu(*head, args.frames, pts[2:3], ref, active=alloc, mask=m)
        wall1 = time.perf_counter() - t0
        ms1 = R.rx_profile_kernel_ms()
        t0 = time.perf_counter()
        prof = R.rx_profile_pa_gpu(*head, args.frames, pts, ref, active=alloc, mask=m)
        wall4 = time.perf_counter() - t0
        ms4 = R.rx_profile_kernel_ms()
        assert np.array_equal(prof.bit_err[0], alone.bit_err)            # the linear point is the plain call
        assert np.array_equal(prof.bit_err[2], one.bit_err[0])           # a point does not care what shares its call
        emit({
            "what": "wofdm_rx_profile_pa N=256 16-QAM CPW half-band %s, points %s, back-off from the mean power %s: "
                    "%d cells x %d frames x %d symbols" % (name, [tuple(q) for q in pts], np.round(ref, 7).tolist(), cells,
                                                           args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames_one_point": R.rx_profile_pa_chunk_frames(st, S, m is not None, 1),
            "chunk_frames_four_points": R.rx_profile_pa_chunk_frames(st, S, m is not None, 4),
            "chunk_frames_plain_call": R.rx_profile_chunk_frames(st, S, m is not None),
            "plain_call_wall_s": wall0, "plain_call_kernels_s": ms0 * 1e-3,
            "one_point_wall_s": wall1, "one_point_kernels_s": ms1 * 1e-3, "one_point_over_plain_kernels": ms1 / ms0,
            "four_points_wall_s": wall4, "four_points_kernels_s": ms4 * 1e-3, "four_points_over_plain_kernels": ms4 / ms0,
            "additional_point_in_plain_calls": (ms4 - ms1) / 3.0 / ms0,
            "frame_points_per_s_kernels": cells * args.frames * 4 / (ms4 * 1e-3),
            "ber_per_point": (prof.bit_err.sum(axis=(1, 2, 3, 4)) / (prof.decisions.sum() * cells * k)).round(5).tolist(),
            "output_over_input_power_per_point": (prof.pa_power[..., 1].sum(axis=(1, 2, 3)) /
                                                  prof.pa_power[..., 0].sum(axis=(1, 2, 3))).round(4).tolist()})
    if not args.physical:
        return
    # the RC pair, plain against masked, without an amplifier and at three back-offs behind the Rapp model
    ibos = [9.0, 6.0, 3.0]
    ppts = [R.PaPoint(R.PA_LINEAR, 0.0)] + [R.PaPoint(R.PA_RAPP, ibo, 2.0) for ibo in ibos]
    symbols = np.random.RandomState(7).choice(T.SYMBOLS_16QAM, size=(n // 2, T.NO_SYMBOLS), replace=True)
    grid = np.zeros((T.NO_SYMBOLS, n), np.complex64)
    grid[:, alloc] = symbols.T
    unloaded = np.fft.fftshift(np.repeat(~alloc, 8))
    res = {}
    for name, m in (("plain", None), ("masked", mask)):
        ref = R.pa_ref_power(st, k, S, w_tx[:1], 3, 0, 200, active=alloc, mask=m)
        prof = R.rx_profile_pa_gpu(st, k, S, w_tx[:1], w_rx[:1], h, [30.0], 3, 0, args.physical_frames, ppts, ref, active=alloc,
                                   mask=m)
        dec = n_ch * args.physical_frames * (S - 1) * int(np.count_nonzero(alloc))
        psd = T.tx_psd_batch_gpu(n, grid[None], [(0, st.cp, st.cs, st.tail_tx, w_tx[0], m, q) for q in ppts])
        res[name] = {"ser": (prof.sym_err.sum(axis=(1, 2, 3, 4)) / dec).round(5).tolist(),
                     "evm_db": (10 * np.log10(prof.err_power.sum(axis=(1, 2, 3, 4)) / dec)).round(2).tolist(),
                     "obr_over_inband_db": (10 * np.log10(psd[:, unloaded].mean(axis=1) / psd[:, ~unloaded].mean(axis=1))).round(2).tolist()}
    emit({"what": "RC pair, CPW N=256 cp=32 half band, 16-QAM at 30 dB, 4 Veh-A channels x %d frames; OBR of 256 symbols: "
                  "no amplifier, then Rapp p = 2 at %s dB of back-off" % (args.physical_frames, ibos), **res})


if __name__ == "__main__":
    main()
