#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_tx_papr on a CCDF-sized job -- 72 window pairs x 10^5 frames x 16 symbols at
N = 256, 16-QAM, half-band loading (wtx, CP 32: 72 random Tx windows), once plain and once with the reference's Tx mask.

Per run: host wall clock around the whole call (allocations, uploads, the mask's preparation and the copy-back
included), the kernels' share of it (HIP events around the chunk loop, wofdm_tx_papr_kernel_ms) and symbol periods per
second by both clocks; also the rate of the fp64 host mirror (timefreq.frame_papr) on a few frames.  One JSON line per
run, after one small warm-up call.

    python tools/bench_tx_papr.py [--frames 100000] [--pairs 72]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wofdm_amd import _lib  # noqa: E402
from wofdm_amd import channel_mask as CM  # noqa: E402
from wofdm_amd import timefreq as T  # noqa: E402
from wofdm_amd import variants as V  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--pairs", type=int, default=72)
    args = ap.parse_args()
    n, k, S = 256, 4, 16
    st = V.make_structure("wtx", n, 32)
    rs = np.random.RandomState(0)
    w = np.stack([V.expand_tx_window(st, np.concatenate(([1.0], np.sort(rs.uniform(0.02, 0.98, st.tail_tx))[::-1])))
                  for _ in range(args.pairs)])
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    tab = T.qam_table(k)
    grids = tab[rs.randint(0, tab.size, size=(8, S, n))] * alloc[None, None, :]
    for name, m in (("plain", None), ("masked", mask)):
        T.tx_papr_gpu(st, k, S, w, 1, 0, 64, active=alloc, mask=m)                    # warm-up
        t0 = time.perf_counter()
        hist, mx = T.tx_papr_gpu(st, k, S, w, 1, 0, args.frames, active=alloc, mask=m)
        wall = time.perf_counter() - t0
        ms = C.c_float(0.0)
        _lib.check(_lib.load().wofdm_tx_papr_kernel_ms(C.byref(ms)))
        periods = args.pairs * args.frames * S
        assert int(hist.sum()) == periods
        t0 = time.perf_counter()
        T.frame_papr(st, grids, w[0], m)
        host = (time.perf_counter() - t0) / (8 * S)
        ccdf = T.papr_ccdf(hist.sum(axis=0))
        print(json.dumps({
            "what": "wofdm_tx_papr N=256 16-QAM half-band %s: %d pairs x %d frames x %d symbols" % (name, args.pairs, args.frames, S),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": T.tx_papr_chunk_frames(st, S, m is not None), "wall_s": wall, "kernels_s": ms.value * 1e-3,
            "kernel_share": ms.value * 1e-3 / wall, "periods": periods, "periods_per_s_wall": periods / wall,
            "periods_per_s_kernels": periods / (ms.value * 1e-3), "host_mirror_periods_per_s": 1.0 / host,
            "max_papr_db": float(10 * np.log10(mx.max())),
            "papr_db_at_ccdf_1e-3": float(0.25 * np.argmax(ccdf < 1e-3)) if (ccdf < 1e-3).any() else None}), flush=True)


if __name__ == "__main__":
    main()
