#!/usr/bin/env python3
"""Developer tool (GPU box): time wofdm_rx_profile_tracking beside wofdm_rx_profile_soft with the same link point, in ONE run -- the
shape of tools/bench_rx_profile_soft.py: the half-band system of main_channel_mask.m at N = 256, 16-QAM, 16 symbols per frame
(CPW, CP 32), 2 window pairs x 8 SNR points x 4 Veh-A channels = 64 cells, once plain and once with the reference's Tx mask.
Pair 0 is the raised-cosine pair, pair 1 a pair with linear edges (the same tails, straight ramps).

Per run, the kernels' time (HIP events around the chunk loop, wofdm_rx_profile_kernel_ms).  The calls of a run are made in
rounds -- every variant once per round, --rounds rounds after a warm-up round --, so that a drift of the clocks meets every
variant alike; per variant the median, the smallest and the largest of its rounds are reported, and the soft call's own spread is
what a difference has to exceed to mean anything:
  - the link point is the one a tracking receiver is for: a free-running carrier offset of 0.02 with a linewidth of 1e-3,
    free-running as well;
  - wofdm_rx_profile_soft, and wofdm_rx_profile_tracking with the receivers (0, 0), (1, 0), (0, 1), (1, 1) behind a comb on every
    eighth loaded bin, each with one and with sixteen scales (the first of the default half-octave list).
The (0, 0) receiver's per-bin fields are compared with the soft call's on the data bins by bytes on the way.  With sixteen scales
the run also reports, per receiver, the symbol-error rate and the achievable rate (``gmi``, a scale per bin) over the cells, per
pair.  One JSON line per run.  A diagnostic route, not the hot path; the boxes switch clock states, so only figures of one run
compare.

    python tools/bench_rx_profile_tracking.py [--frames 2000] [--rounds 5]
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

RECEIVERS = ((0, 0), (1, 0), (0, 1), (1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    n, k, S, n_ch = 256, 4, 16, 4
    st = W.make_structure("CPW", n, 32)
    h = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"][:n_ch].astype(np.complex64)
    snr = np.arange(0.0, 32.0, 4.0, dtype=np.float32)
    lin_tx = W.expand_tx_window(st, np.concatenate(([1.0], np.linspace(1.0, 0.0, st.tail_tx + 2)[1:-1])))
    lin_rx = W.expand_rx_window(st, np.concatenate(([1.0], np.linspace(0.5, 0.0, st.tail_rx // 2 + 2)[1:-1])))
    names = ("rc", "linear")
    w_tx = np.stack([W.tx_rc_window(st), lin_tx]).astype(np.float32)
    w_rx = np.stack([W.rx_rc_window(st), lin_rx]).astype(np.float32)
    alloc, mask = CM.half_band_allocation(n), CM.tx_mask(st.sym_len)
    pil = R.pilot_comb(alloc, 8)
    data = alloc & ~pil
    point = R.LinkPoint(cfo=0.02, cfo_tracked=0, linewidth=1e-3, cpe_tracked=0)
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
        variants = {}
        for ns in (1, 16):
            sc = R.SOFT_SCALES[:ns]
            variants["soft_%d_scales" % ns] = lambda f, sc=sc: R.rx_profile_soft_gpu(*base, f, [point], sc, **kw)
            for cpe, post in RECEIVERS:
                variants["tracking_%d%d_%d_scales" % (cpe, post, ns)] = (
                    lambda f, sc=sc, tp=(cpe, post): R.rx_profile_tracking_gpu(*base, f, [point], [tp], pil, sc, **kw))
        ms, last = {v: [] for v in variants}, {}
        for call in variants.values():
            call(8)                                                        # warm-up
        for rnd in range(args.rounds + 1):
            for v, call in variants.items():
                last[v] = call(args.frames)
                if rnd > 0:
                    ms[v].append(R.rx_profile_kernel_ms())
        res = {}
        for ns in (1, 16):
            soft = float(np.median(ms["soft_%d_scales" % ns]))
            for v in [v for v in variants if v.endswith("_%d_scales" % ns)]:
                a = np.asarray(ms[v])
                res[v + "_kernels_ms"] = {"median": round(float(np.median(a)), 2), "min": round(float(a.min()), 2),
                                          "max": round(float(a.max()), 2)}
                if v.startswith("tracking"):
                    res[v + "_over_soft"] = round(float(np.median(a)) / soft, 4)
            s0, t0 = last["soft_%d_scales" % ns], last["tracking_00_%d_scales" % ns]
            for f in ("bit_err", "sym_err", "err_power", "bit_penalty"):
                assert (np.ascontiguousarray(getattr(s0, f)[..., data]).tobytes()
                        == np.ascontiguousarray(getattr(t0, f)[..., data]).tobytes()), f
        for cpe, post in RECEIVERS:
            prof = last["tracking_%d%d_16_scales" % (cpe, post)]
            dec = float(prof.decisions[0].sum())
            ser = (prof.sym_err[0].sum(axis=-1) / dec).mean(axis=(1, 2))
            rate = R.gmi(prof, k)[0][0].mean(axis=(1, 2))
            res["receiver_%d%d" % (cpe, post)] = {"symbol_error_rate": dict(zip(names, np.round(ser, 4).tolist())),
                                                  "rate_bit_per_decision": dict(zip(names, np.round(rate, 4).tolist()))}
        print(json.dumps(dict({
            "what": "wofdm_rx_profile_tracking N=256 16-QAM CPW half-band %s (gamma = %d, B = %d): %d cells x %d frames x %d symbols, "
                    "one point (cfo 0.02 and linewidth 1e-3, both free-running), %d pilot bins of %d loaded, %d rounds"
                    % (name, st.prefix_rm, st.stride, cells, args.frames, S, int(pil.sum()), int(alloc.sum()), args.rounds),
            "device": dev, "when": time.strftime("%Y-%m-%d %H:%M:%S %Z"),
            "chunk_frames": R.rx_profile_tracking_chunk_frames(st, S, m is not None, 1, False, 16)}, **res)), flush=True)


if __name__ == "__main__":
    main()
