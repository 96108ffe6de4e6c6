#!/usr/bin/env python3
"""Developer tool (GPU box): how evenly one launch of the benchmark's shape loads its workgroups, from the WOFDM_STAMP
diagnostic build (the totals tools/stamp_report.py splits by phase).

    WOFDM_LIB=$PWD/ab/lib_stamp.so python tools/work_split_report.py [N] [K]

A wave's stamped cycles are its time inside the frame loop (loop control and chunk grabs included), so the largest total is the
length of the launch and largest / mean is the share of wave-slot time an even end would give back.  profiles/work_split.txt.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import wofdm_amd as W  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
k = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ch = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "channels_vehA.npz"))["h"]
st = W.make_structure("wtx" if n <= 256 else "WOLA", n, 32)
snr = np.arange(-5.0, 51.0, 5.0).astype(np.float32)
cfg = W.make_cfg(st, k, 16, 21, 1, 12, 1, noise_before_truncate=True, seed=2)
frames = 62500 * 256 // n
with W.Plan(cfg, W.tx_rc_window(st), W.rx_rc_window(st), ch[:1].astype(np.complex64), snr) as plan:
    info = plan.info()
    grid, waves, occ = info["workgroups"], info["waves_per_workgroup"], info["workgroups_per_cu"]
    buf = torch.zeros(4 * 12 + grid * 16 * 16, dtype=torch.int64, device="cuda")
    plan.launch_timed(0, frames, buf)                # (warm-up: code object, clocks)
    buf.zero_()
    ms = plan.launch_timed(0, frames, buf)
    torch.cuda.synchronize()
    st_ = buf[48:].cpu().numpy().reshape(grid, 16, 16)[:, :waves, :].astype(np.float64)
tot = st_.sum(axis=2)                                # [workgroup][wave] in-loop cycles
wg = tot.max(axis=1)                                 # a workgroup holds its slots until its last wave is through
q = np.percentile(wg, [0, 25, 50, 75, 100])
print("N=%d k=%d: %.3f ms, %d workgroups (%d per CU) x %d waves" % (n, k, ms, grid, occ, waves))
print("  in-loop cycles per wave: mean %.4e  max %.4e  max/mean %.4f" % (tot.mean(), tot.max(), tot.max() / tot.mean()))
print("  per workgroup (its slowest wave): min %.4e  q1 %.4e  median %.4e  q3 %.4e  max %.4e" % tuple(q))
print("  spread (max - min) / max %.4f;  slot time used = mean / max %.4f" % ((q[4] - q[0]) / q[4], wg.mean() / wg.max()))
