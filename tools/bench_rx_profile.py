#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile beside Plan.launch on the same cells -- the half-band system of
main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame (CPW, CP 32): 2 window pairs x 8 SNR points x 4 Veh-A
channels = 64 cells, once plain and once with the reference's Tx mask.

Per run: host wall clock around the whole call (allocations, uploads, the mask's preparation and the copy-back included),
the kernels' share of it (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms), frames per second by both clocks,
and for scale the frame kernel's time for the same cells and frames (Plan.launch_timed; it counts per cell, not per bin).
One JSON line per run, after one small warm-up call.  The profile is a diagnostic route, not the hot path.

    python tools/bench_rx_profile.py [--frames 2000]
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
    cells = pairs * snr.size * n_ch
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    for name, m in (("plain", None), ("masked", mask)):
        R.rx_profile_gpu(st, k, S, w_tx, w_rx, h, snr, 1, 0, 8, active=alloc, mask=m)                 # warm-up
        t0 = time.perf_counter()
        prof = R.rx_profile_gpu(st, k, S, w_tx, w_rx, h, snr, 1, 0, args.frames, active=alloc, mask=m)
        wall = time.perf_counter() - t0
        ms = R.rx_profile_kernel_ms()
        cfg = W.make_cfg(st, k, S, h.shape[1], n_ch, snr.size, pairs, seed=1)
        with W.Plan(cfg, w_tx, w_rx, h, snr) as plan:
            plan.set_allocation(alloc)
            if m is not None:
                plan.set_tx_mask(m)
            counts = plan.new_counts()
            plan.launch_timed(0, 8, counts)                                                           # warm-up
            counts.zero_()
            plan_ms = plan.launch_timed(0, args.frames, counts)
            got = counts.cpu().numpy().view(np.uint64)
            kid = plan.kernel_id()
        frames = cells * args.frames
        print(json.dumps({
            "what": "wofdm_rx_profile N=256 16-QAM CPW half-band %s: %d cells x %d frames x %d symbols" % (name, cells, args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": R.rx_profile_chunk_frames(st, S, m is not None), "wall_s": wall, "kernels_s": ms * 1e-3,
            "kernel_share": ms * 1e-3 / wall, "frames": frames, "frames_per_s_wall": frames / wall,
            "frames_per_s_kernels": frames / (ms * 1e-3), "plan_launch_kernel_s": plan_ms * 1e-3, "plan_kernel_id": kid,
            "profile_over_plan": ms / plan_ms,
            "bit_errors_profile": int(prof.bit_err.sum()), "bit_errors_plan": int(got[..., 0].sum())}), flush=True)


if __name__ == "__main__":
    main()
