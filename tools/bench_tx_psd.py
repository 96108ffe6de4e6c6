#!/usr/bin/env python3
"""Developer tool (GPU box): time the N = 256 `-m run_timefreq` sweep -- 6 systems x 12 CPs x 3 windows = 216
averaged periodograms of 256 16-QAM symbols each -- three ways:

  batch   one wofdm_tx_psd_batch call for all 216 (timefreq.tx_psd_batch_gpu)
  single  216 wofdm_tx_psd calls (timefreq.psd_estimate_gpu, the N <= 256 route of estimate_obr)
  numpy   the host mirror, psd_estimate(overlap_and_add(tx_symbols(...)))

Host wall clock around each whole route (every call ends in a device synchronise), best of --reps after one
warm-up.  Prints one JSON line.

    python tools/bench_tx_psd.py [--reps 5]

--masked: wofdm_tx_psd_batch_masked instead.  Two sets -- the N = 256 `run_timefreq`-sized one (6 systems x 4 CPs x 3
windows = 72 jobs x 256 symbols) and an N = 1024 one (the same 72 jobs at N = 1024) -- each timed once unmasked
(wofdm_tx_psd_batch) and once with every job masked by the reference's mask of its P; wall time per call, the host
preparation of the masks, hipMalloc / hipFree and the copies included, one JSON line per set.  The kernel times come
from the same run under `rocprofv3 --kernel-trace --stats -- python tools/bench_tx_psd.py --masked`
(profiles/tx_psd_masked.txt holds both).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wofdm_amd import timefreq as T  # noqa: E402
from wofdm_amd import variants as V  # noqa: E402

SYSTEMS = ("wtx", "CPwtx", "wrx", "CPwrx", "CPW", "WOLA")       # wofdm_optimization.py defaults
CPS = tuple(range(10, 33, 2))


def sweep(n=256, seed=0):
    rs = np.random.RandomState(seed)
    items = []
    for system in SYSTEMS:
        for cp in CPS:
            st = V.make_structure(system, n, cp)
            w_tx = V.tx_rc_window(st)
            items.append((st, T.draw_symbols(n, rs), T._obr_windows(st, w_tx)))
    return items


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def masked_sets(reps):
    from wofdm_amd import channel_mask as CM
    for n in (256, 1024):
        rs = np.random.RandomState(1)
        grids, jobs = [], []
        for system in SYSTEMS:
            for cp in (10, 16, 24, 32):
                st = V.make_structure(system, n, cp)
                for w, ov in T._obr_windows(st, V.tx_rc_window(st)):
                    jobs.append((len(grids), st.cp, st.cs, ov, w))
                grids.append(T._full_grid(n, T.draw_symbols(n, rs)))
        grids = np.stack(grids)
        assert len(jobs) == 72
        masked = [j + (CM.tx_mask(n + j[1] + j[2]),) for j in jobs]
        res = {"what": "N=%d, 72 jobs x 256 symbols" % n, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
               "distinct_masks": len({n + j[1] + j[2] for j in jobs}),
               "unmasked_wall_s": best(lambda: T.tx_psd_batch_gpu(n, grids, jobs), reps),
               "masked_wall_s": best(lambda: T.tx_psd_batch_gpu(n, grids, masked), reps)}
        res["masked_over_unmasked"] = res["masked_wall_s"] / res["unmasked_wall_s"]
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--masked", action="store_true")
    args = ap.parse_args()
    if args.masked:
        return masked_sets(args.reps)
    n = 256
    items = sweep(n)
    grids = np.stack([T._full_grid(n, X) for _, X, _ in items])
    jobs = [(b, st.cp, st.cs, ov, w) for b, (st, _, wins) in enumerate(items) for w, ov in wins]
    assert len(jobs) == 216

    def batch():
        return T.tx_psd_batch_gpu(n, grids, jobs)

    def single():
        return [T.psd_estimate_gpu(st, X, w, ov) for st, X, wins in items for w, ov in wins]

    def host():
        return [T.psd_estimate(T.overlap_and_add(T.tx_symbols(st, X, w), ov), 8 * n)
                for st, X, wins in items for w, ov in wins]

    a, b = np.asarray(batch()), np.asarray(single())
    dev = "?"
    try:
        import torch
        dev = torch.cuda.get_device_name(0)
    except Exception:                       # noqa: BLE001  (the name is a label only)
        pass
    res = {"what": "N=256 run_timefreq sweep, 216 periodograms", "device": dev,
           "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
           "batch_s": best(batch, args.reps), "single_s": best(single, args.reps),
           "numpy_s": best(host, max(1, args.reps // 2)),
           "batch_vs_single_max_rel": float(np.abs(a - b).max() / b.max())}
    res["single_over_batch"] = res["single_s"] / res["batch_s"]
    res["numpy_over_batch"] = res["numpy_s"] / res["batch_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
